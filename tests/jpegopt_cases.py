"""The cases of the optimised-Huffman tests (test_jpegopt_host.py, test_gpu_jpegopt.py, golden/make_jpegopt_golden.py): every case
of jpeg_cases.CASES, one image that forces the length limiting, and synthetic histograms for the table construction.  The
restatement's results are computed once per process; host_results() builds tests/jpegopt_host.cpp and runs it as a process of its own."""
import atexit
import functools
import os
import shutil
import struct
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

import jpeg_cases
import jpeg_ref as ref
import jpegd_cases
import jpegopt_ref as oref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_opt_streams.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegopt_host.cpp')

LIMITED = jpeg_cases.Case('limited_128x192_q100_444', ('limited',), 128, 192, 100, '4:4:4', False)
CASES = list(jpeg_cases.CASES) + [LIMITED]
IDS = [c.name for c in CASES]


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def build(case):
    """uint8 (n, h, w, 3), read-only."""
    if case is not LIMITED:
        return jpeg_cases.build(case)
    h, w = case.h, case.w
    rng = np.random.default_rng(1)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    amp = 127 * np.exp(-4 * x / w)              # noise that fades to the right: a few very frequent and many very rare AC symbols
    img = np.clip(np.rint(128 + amp[..., None] * rng.uniform(-1, 1, (h, w, 3))), 0, 255).astype(np.uint8)[None]
    img.setflags(write=False)
    return img


Reference = namedtuple('Reference', 'coefs flat hists tables files ecds')


@functools.lru_cache(maxsize=None)
def reference(case):
    """The restatement's results for a case: per image the coefficients, their flat device layout (n, blocks * 64), the histograms
    (n, 4, 257), the optimal tables (n, 4, 272), the whole files and their entropy-coded segments."""
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    coefs = jpeg_cases.reference(case).coefs if case is not LIMITED else [ref.coefficients(img, case.quality, hs, vs) for img in build(case)]
    done = [oref.encode(c, case.h, case.w, case.quality, hs, vs) for c in coefs]
    return Reference(coefs, np.stack([ref.flat_coefficients(c) for c in coefs]), np.stack([d[2] for d in done]),
                     np.stack([d[1] for d in done]), [d[0] for d in done], [d[3] for d in done])


@functools.lru_cache(maxsize=None)
def golden():
    """golden/jpeg_opt_streams.npz taken apart: case name -> [Pillow's optimize=True file per image]."""
    z = np.load(GOLDEN)
    ends = np.concatenate([[0], z['file_ends']])
    blob = z['files'].tobytes()
    out, k = {}, 0
    for name in z['names'].tolist():
        n = len(jpeg_cases.by_name(name).contents)
        out[name] = [blob[ends[k + i]:ends[k + i + 1]] for i in range(n)]
        k += n
    return out


# ---- synthetic histograms --------------------------------------------------------------------------------------------------
def _fibonacci(count):
    f = [1, 2]                                  # with the pseudo-symbol of weight 1 in front: every merge deepens one chain
    while len(f) < count:
        f.append(f[-1] + f[-2])
    return f[:count]


@functools.lru_cache(maxsize=None)
def synthetic():
    """(names, histograms (m, 257) uint32, read-only)."""
    names, rows = [], []

    def add(name, values):
        row = np.zeros(257, np.uint32)
        for k, v in values.items():
            row[k] = v
        names.append(name)
        rows.append(row)

    add('single', {0x21: 1000})
    add('two-equal', {3: 7, 200: 7})
    add('twelve-dc', {k: 40 for k in range(12)})
    for count in (20, 24, 30):                                # code sizes 20, 24, 30: the limiting loop runs many times
        add('fibonacci-{}'.format(count), {3 * k + 1: f for k, f in enumerate(_fibonacci(count))})
    add('fibonacci-40', {5 * k + 2: f for k, f in enumerate(_fibonacci(40))})       # a code size above 32: status 1
    add('total-2^32', {17: 1 << 31, 18: 1 << 31})                                   # status 2
    add('total-2^32-1', {17: 1 << 31, 18: (1 << 31) - 1})                           # with the pseudo-symbol 2^32 as well
    add('total-2^32-2', {17: 1 << 31, 18: (1 << 31) - 2})                           # the largest total that is coded
    add('zeros', {})
    rng = np.random.default_rng(20250119)
    for k in range(200):
        row = np.floor(2.0 ** rng.uniform(0, 24, 256)).astype(np.uint32)
        row[rng.uniform(size=256) < rng.uniform()] = 0
        add('random-{}'.format(k), dict(enumerate(row.tolist())))
    out = np.stack(rows)
    out.setflags(write=False)
    return names, out


@functools.lru_cache(maxsize=None)
def synthetic_reference():
    """((m, 272) tables, (m,) status) of the restatement."""
    return oref.optimal_tables(synthetic()[1])


# ---- the host program ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(sanitize):
    """Builds tests/jpegopt_host.cpp once per process into a temporary directory, removed when the process ends."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegopt_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegopt_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


Image = namedtuple('Image', 'h w hs vs coef')            # coef: the flat int16 device layout of one image
HostImage = namedtuple('HostImage', 'hist tables status valid codes')


def host_results(hists, images, given, sanitize=True):
    """Runs the host program: the table construction over `hists` (m, 257); for every Image its histograms, their optimal tables and
    the validate-and-derive step on them; validate-and-derive on each (4, 272) set of `given`.  Returns ((m, 272) tables, (m,) status,
    [HostImage], [(valid, codes (544,))], the completed process)."""
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegopt_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<3I', len(hists), len(images), len(given)))
            f.write(np.ascontiguousarray(hists, np.uint32).tobytes())
            for im in images:
                f.write(struct.pack('<4iI', im.h, im.w, im.hs, im.vs, len(im.coef)) + np.ascontiguousarray(im.coef, np.int16).tobytes())
            for t in given:
                f.write(np.ascontiguousarray(t, np.uint8).tobytes())
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)
        if done.returncode != 0:
            return None, None, None, None, done
        blob = open(os.path.join(work, 'out.bin'), 'rb').read()
        m, at = len(hists), 0
        tables = np.frombuffer(blob, np.uint8, m * 272, at).reshape(m, 272)
        at += m * 272
        status = np.frombuffer(blob, np.uint32, m, at).astype(np.int64)
        at += 4 * m
        out = []
        for _ in images:
            hist = np.frombuffer(blob, np.uint32, 4 * 257, at).reshape(4, 257)
            at += 4 * 4 * 257
            tabs = np.frombuffer(blob, np.uint8, 4 * 272, at).reshape(4, 272)
            at += 4 * 272
            st = np.frombuffer(blob, np.uint32, 5, at)
            at += 20
            codes = np.frombuffer(blob, np.uint32, 544, at)
            at += 4 * 544
            out.append(HostImage(hist, tabs, st[:4].astype(np.int64), int(st[4]), codes))
        derived = []
        for _ in given:
            valid = struct.unpack_from('<I', blob, at)[0]
            derived.append((valid, np.frombuffer(blob, np.uint32, 544, at + 4)))
            at += 4 + 4 * 544
        assert at == len(blob)
        return tables, status, out, derived, done
    finally:
        shutil.rmtree(work, ignore_errors=True)


def code_words(tables):
    """The restatement's form of the derive step: (4, 272) -> (valid, (544,) uint32: symbol -> code << 5 | length, laid out
    Y DC [16] | chroma DC [16] | Y AC [256] | chroma AC [256]; all zero when not valid)."""
    out = np.zeros(544, np.uint32)
    base = (0, 32, 16, 288)
    parts = [oref.codes_of(tables[t], t % 2 == 0) for t in range(4)]
    if not all(ok for _, ok in parts):
        return 0, out
    for t, (codes, _) in enumerate(parts):
        for sym, (code, length) in codes.items():
            out[base[t] + sym] = code << 5 | length
    return 1, out
