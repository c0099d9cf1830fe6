"""The cases of the progressive-JPEG tests (test_jpegprog_host.py, test_gpu_jpegprog.py, golden/make_jpegprog_golden.py): the golden
images of jpeg_cases at their sub-samplings, a ragged size under restart intervals, caller's quantisation tables, a crafted image
whose correction bits force the 937-bit flush, a flat image of 32768 luma blocks (the 0x7fff flush), and synthetic coefficient
tensors for the paths natural images do not reach.  The restatement's results are computed once per process; host_results() builds
tests/jpegprog_host.cpp and runs it as a process of its own."""
import atexit
import functools
import os
import shutil
import struct
import subprocess
import tempfile
import zlib
from collections import namedtuple

import numpy as np

import jpeg_cases
import jpeg_ref as ref
import jpegd_cases
import jpegprog_ref as pref
import jpegq_cases
import jpegq_ref as qref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpegprog_streams.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegprog_host.cpp')

# kind: 'jpeg' = the images of jpeg_cases.by_name(arg) | 'image' = one jpeg_cases image of content arg | 'corr' = the crafted grey
# image | 'flat' = a constant.  qtables: None or a kind of jpegq_cases.tables.  slow: the restatement takes seconds on it (32768 blocks
# in plain Python) - test_jpegprog_host.py runs it once, the GPU tests hold the device to the host program and Pillow's file there.
Case = namedtuple('Case', 'name kind arg h w quality subsampling ri qtables slow')


def _cases():
    out = []
    for c in jpeg_cases.GOLDEN_CASES:
        out.append(Case('g_' + c.name, 'jpeg', c.name, c.h, c.w, c.quality, c.subsampling, 0, None, False))
    for ss in jpeg_cases.SUBSAMPLINGS:                       # 37x53 at 4:2:0: 7 real luma block columns against 8 in the MCU grid
        for ri in (0, 1, 2, 3, 7):
            out.append(Case('mixed_37x53_q75_{}_ri{}'.format(ss.replace(':', ''), ri), 'image', 'mixed', 37, 53, 75, ss, ri, None, False))
    out.append(Case('smooth_37x53_q30_420_ri3', 'image', 'smooth', 37, 53, 30, '4:2:0', 3, None, False))
    out.append(Case('mixed_40x56_random_420', 'image', 'mixed', 40, 56, None, '4:2:0', 0, 'random', False))
    out.append(Case('mixed_17x33_three_444_ri2', 'image', 'mixed', 17, 33, None, '4:4:4', 2, 'three', False))
    out.append(Case('mixed_40x56_three_422', 'image', 'mixed', 40, 56, None, '4:2:2', 0, 'three', False))
    # more than 256 blocks in a scan: the runs are resolved 256 summaries at a time, and a run or a restart interval crosses the seam
    out.append(Case('mixed_128x192_q75_420_ri5', 'image', 'mixed', 128, 192, 75, '4:2:0', 5, None, False))
    out.append(Case('smooth_136x200_q95_444', 'image', 'smooth', 136, 200, 95, '4:4:4', 0, None, False))
    out.append(Case('corr_32x160_q100_444', 'corr', None, 32, 160, 100, '4:4:4', 0, None, False))
    out.append(Case('corr_32x160_q100_420', 'corr', None, 32, 160, 100, '4:2:0', 0, None, False))
    out.append(Case('corr_32x160_q100_444_ri7', 'corr', None, 32, 160, 100, '4:4:4', 7, None, False))
    out.append(Case('flat_512x4096_q75_444', 'flat', None, 512, 4096, 75, '4:4:4', 0, None, True))
    return out


CASES = _cases()
QUICK = [c for c in CASES if not c.slow]
IDS = [c.name for c in CASES]


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def build(case):
    """uint8 (n, h, w, 3), read-only."""
    if case.kind == 'jpeg':
        return jpeg_cases.build(jpeg_cases.by_name(case.arg))
    if case.kind == 'image':
        x = jpeg_cases._image(case.arg, case.h, case.w, zlib.crc32(case.name.encode()))[None]
    elif case.kind == 'flat':
        x = np.broadcast_to(np.array([200, 17, 96], np.uint8), (1, case.h, case.w, 3)).copy()
    else:
        # every luma block the inverse DCT of 63 AC coefficients of +-6: at quality 100 every one of them is a correction bit of both
        # luma refine scans and no block has a new coefficient, so 63 bits per block wait for the end of the run
        rng = np.random.default_rng(937)
        coef = np.zeros((case.h // 8, case.w // 8, 64), np.int64)
        coef[..., 1:] = 6 * rng.choice([-1, 1], coef[..., 1:].shape)
        grey = ref.idct(coef.reshape(case.h // 8, case.w // 8, 8, 8)).transpose(0, 2, 1, 3).reshape(case.h, case.w)
        x = np.repeat(grey.astype(np.uint8)[..., None], 3, -1)[None]
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def qtables(case):
    return None if case.qtables is None else jpegq_cases.tables(case.qtables)


def coefficients(case, img):
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    qt = qtables(case)
    return ref.coefficients(img, case.quality, hs, vs) if qt is None else qref.coefficients(img, qt, hs, vs)


def baseline_header(case):
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    qt = qtables(case)
    return ref.header(case.h, case.w, case.quality, hs, vs) if qt is None else qref.header(case.h, case.w, qt, hs, vs)


Reference = namedtuple('Reference', 'coefs flat hists tables files segments stats')


@functools.lru_cache(maxsize=None)
def reference(case):
    """The restatement's results for a case: per image the coefficients, their flat device layout (n, blocks * 64), the histograms
    (n, 10, 257), the optimal tables (n, 10, 272), the whole files, their ten segments; and the path counters summed over the batch."""
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    stats = {}
    coefs = [coefficients(case, img) for img in build(case)]
    prefix = pref.prefix_of(baseline_header(case))
    done = [pref.encode(c, case.h, case.w, hs, vs, prefix, case.ri, stats) for c in coefs]
    return Reference(coefs, np.stack([ref.flat_coefficients(c) for c in coefs]), np.stack([d[2] for d in done]),
                     np.stack([d[1] for d in done]), [d[0] for d in done], [d[3] for d in done], stats)


@functools.lru_cache(maxsize=None)
def flat(case):
    """(n, blocks * 64) int16 without the restatement's coder: what a slow case needs."""
    return np.stack([ref.flat_coefficients(coefficients(case, img)) for img in build(case)])


@functools.lru_cache(maxsize=None)
def golden():
    """golden/jpegprog_streams.npz taken apart: case name -> [Pillow's progressive=True file per image]."""
    z = np.load(GOLDEN)
    ends = np.concatenate([[0], z['file_ends']])
    blob = z['files'].tobytes()
    out, k = {}, 0
    for name in z['names'].tolist():
        n = len(build(by_name(name)))
        out[name] = [blob[ends[k + i]:ends[k + i + 1]] for i in range(n)]
        k += n
    return out


def split_file(data):
    """A progressive file -> (tables (10, 272) in DHT order, [10 entropy-coded segments]) by its markers alone."""
    tables, segs, i = [], [], 2
    while data[i:i + 2] != b'\xff\xd9':
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], 'big')
        if marker == 0xc4:
            t = np.zeros(272, np.uint8)
            body = data[i + 5:i + 2 + length]
            t[:len(body)] = list(body)
            tables.append(t)
        i += 2 + length
        if marker == 0xda:
            j = i
            while not (data[j] == 0xff and data[j + 1] != 0 and not 0xd0 <= data[j + 1] <= 0xd7):
                j += 1
            segs.append(data[i:j])
            i = j
    return np.stack(tables), segs


# ---- synthetic coefficient tensors --------------------------------------------------------------------------------------------------
Synthetic = namedtuple('Synthetic', 'name h w hs vs ri flat')


def coefs_of_flat(flat_coef, h, w, hs, vs):
    comps, _ = ref.geometry(h, w, hs, vs)
    out, at = [], 0
    for _, _, bh, bw in comps:
        out.append(np.asarray(flat_coef[at:at + bh * bw * 64]).reshape(bh, bw, 64))
        at += bh * bw * 64
    return out


@functools.lru_cache(maxsize=None)
def synthetic():
    """Coefficient tensors no image gives: values beyond the clamps, long zero runs in front of and behind the new coefficients of a
    refine scan, blocks that are all correction bits between blocks with new coefficients, an empty image."""
    out = []
    for k, (h, w, hs, vs, ri) in enumerate(((16, 24, 1, 1, 0), (37, 53, 2, 2, 0), (24, 40, 2, 1, 3), (16, 16, 2, 2, 1))):
        rng = np.random.default_rng(4100 + k)
        blocks = sum(bh * bw for _, _, bh, bw in ref.geometry(h, w, hs, vs)[0])
        c = np.zeros((blocks, 64), np.int16)
        for b in range(blocks):
            kind = rng.integers(0, 6)
            if kind == 0:                                          # beyond the clamps
                c[b] = rng.choice([-32768, -2048, -1024, 1023, 2047, 32767, 0, 1], 64)
            elif kind == 1:                                        # +-1 far apart: ZRL in the last refine scans, first scans empty
                c[b, rng.choice(np.arange(1, 64), 2, replace=False)] = rng.choice([-1, 1], 2)
            elif kind == 2:                                        # a new coefficient early, a correction bit behind a long zero run
                c[b, 2], c[b, 40 + rng.integers(0, 20)] = rng.choice([-1, 1]), rng.choice([-5, 4, 7])
            elif kind == 3:                                        # corrections only
                c[b, 1:] = rng.choice([-7, -6, 4, 5], 63)
            elif kind == 4:                                        # +-2 and +-3 far apart: ZRL in the first refine scan
                c[b, rng.choice(np.arange(1, 64), 3, replace=False)] = rng.choice([-3, -2, 2, 3], 3)
            c[b, 0] = rng.integers(-1024, 1024) if kind else c[b, 0]
        out.append(Synthetic('synthetic{}_{}x{}_{}{}_ri{}'.format(k, h, w, hs, vs, ri), h, w, hs, vs, ri, c.reshape(-1)))
    out.append(Synthetic('zeros_16x16', 16, 16, 1, 1, 0, np.zeros(12 * 64, np.int16)))
    return out


@functools.lru_cache(maxsize=None)
def synthetic_reference(name):
    """(hist (10, 257), tables (10, 272), [10 segments], stats) of the restatement for one synthetic tensor."""
    s = next(x for x in synthetic() if x.name == name)
    stats = {}
    items = pref.all_items(coefs_of_flat(s.flat, s.h, s.w, s.hs, s.vs), s.h, s.w, s.hs, s.vs, s.ri, stats)
    hist = pref.histograms(items)
    tables, status = pref.opt.optimal_tables(hist)
    assert not status.any()
    segs, st = pref.segments(items, tables, stats)
    assert st == 0
    return hist, tables, segs, stats


# ---- the host program ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(sanitize):
    """Builds tests/jpegprog_host.cpp once per process into a temporary directory, removed when the process ends."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegprog_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegprog_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


Image = namedtuple('Image', 'h w hs vs ri coef tables')           # coef: flat int16; tables: None (its optimal ones) or (10, 272)
HostImage = namedtuple('HostImage', 'hist tables status segments')


def host_results(images, sanitize=True):
    """Runs the host program over the Images -> ([HostImage], the completed process)."""
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegprog_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(images)))
            for im in images:
                f.write(struct.pack('<5i2I', im.h, im.w, im.hs, im.vs, im.ri, int(im.tables is not None), len(im.coef)))
                f.write(np.ascontiguousarray(im.coef, np.int16).tobytes())
                if im.tables is not None:
                    f.write(np.ascontiguousarray(im.tables, np.uint8).tobytes())
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)
        if done.returncode != 0:
            return None, done
        blob = open(os.path.join(work, 'out.bin'), 'rb').read()
        out, at = [], 0
        for _ in images:
            hist = np.frombuffer(blob, np.uint32, 10 * 257, at).reshape(10, 257)
            at += 4 * 10 * 257
            tabs = np.frombuffer(blob, np.uint8, 10 * 272, at).reshape(10, 272)
            at += 10 * 272
            status = struct.unpack_from('<I', blob, at)[0]
            lengths = struct.unpack_from('<10I', blob, at + 4)
            at += 44
            segs = []
            for ln in lengths:
                segs.append(blob[at:at + ln])
                at += ln
            out.append(HostImage(hist, tabs, status, segs))
        assert at == len(blob)
        return out, done
    finally:
        shutil.rmtree(work, ignore_errors=True)
