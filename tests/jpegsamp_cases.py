"""The cases of the tests of the samplings 4:4:0, 4:1:1, 4:1:0, 1x4 and 2x4 (test_jpegsamp_host.py, test_gpu_jpegsamp.py,
golden/make_jpegsamp_golden.py).  A case is one uint8 image rebuilt from a seed, a quality, a sampling and the
variants of the file the golden file holds for it - the files of the test writer (jpegsamp_ref.py):
    plain   baseline, Annex K tables          rst1   restart interval 1 MCU          rstn   an interval that does not divide the MCUs
    opt     baseline, optimal tables          prog   libjpeg's simple progression    progB  jpegdprog_ref.SCRIPT_B, restart interval 2
and, for every scale in 1, 2, 4, 8 that Pillow can be asked for, the pixels Pillow decodes from them.  The sizes are the smallest at
which each piece can go wrong: 1 x 1; 8 x 8; exactly one MCU and two MCUs down (the h1v2 filter crosses a block row); one pixel more than
an MCU each way (17 x 33, 33 x 17); chroma planes of one row, of one and of two columns (the edge rules of both filters, the `> 2` of
h2v1); for 4:1:0 the widths on both sides of that threshold at 1/2 and at 1/4; and 37 x 67 ragged, noise at a low and ramps at a high
quality, which carries every variant.  The restatement's results are computed once per process."""
import atexit
import contextlib
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
import jpegd_ref
import jpegdprog_cases as dpc
import jpegdprog_ref as dprog
import jpegrst_cases as rc
import jpegrst_ref as rref
import jpegsamp_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_sampling.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegsamp_host.cpp')
SCALES = sr.SCALES
REDUCED = (2, 4, 8)
SAMPLINGS = tuple(sr.WIDE)                       # '4:4:0', '4:1:1', '4:1:0', '1x4', '2x4'
VARIED = (37, 67)                                # the size whose files come in every variant
VARIANTS = ('plain', 'rst1', 'rstn', 'opt', 'prog', 'progB')
RSTN = 4                                         # divides the MCUs of VARIED at none of the five samplings
PIXELS_UP_TO = 600                               # Pillow's pixels are held for images of up to so many pixels, the CRC32 of every one
SETTINGS = (32, 2048)                            # the subsequence bits of the status-and-rounds comparisons

Case = namedtuple('Case', 'name content seed h w quality sampling variants')


def _sizes(hs, vs):
    out = [(1, 1), (8, 8), (8 * vs, 8 * hs), (16 * vs, 8 * hs), (17, 33), (33, 17),
           (3 * vs, hs), (vs, 2 * hs), (2 * vs + 1, 3 * hs)]               # chroma of 3 x 1, 1 x 2, 3 x 3 samples
    if (hs, vs) == (4, 2):
        out += [(16, 8), (16, 9), (16, 16), (16, 17)]                       # scaled chroma rows of 2 | 3 samples at 1/2 and at 1/4
    return list(dict.fromkeys(out))


def _cases():
    out = []
    for sampling in SAMPLINGS:
        hs, vs = sr.WIDE[sampling]
        for k, (h, w) in enumerate(_sizes(hs, vs)):
            out.append(_case(('noise', 'mixed')[k % 2], 300 + len(out), h, w, (30, 90)[(k // 2) % 2], sampling))
        out.append(_case('noise', 300 + len(out), VARIED[0], VARIED[1], 30, sampling))
        out.append(_case('mixed', 300 + len(out), VARIED[0], VARIED[1], 90, sampling, VARIANTS))
    return out


def _case(content, seed, h, w, quality, sampling, variants=('plain',)):
    name = '{}_{}x{}_q{}_{}'.format(content, h, w, quality, sampling.replace(':', ''))
    return Case(name, content, seed, h, w, quality, sampling, tuple(variants))


CASES = _cases()
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)


def by_name(name):
    return next(c for c in CASES if c.name == name)


def factors(case):
    return sr.SAMPLINGS[case.sampling]


def askable(case, s):
    """Pillow's draft() reaches scale s only by a requested size of at least one pixel a side."""
    return case.h >= s and case.w >= s


def request(case, s):
    return case.w // s, case.h // s


@functools.lru_cache(maxsize=None)
def build(case):
    x = jpeg_cases._image(case.content, case.h, case.w, case.seed)
    x.setflags(write=False)
    return x


def qtables(case):
    return sr.qtables(case.quality)


@functools.lru_cache(maxsize=None)
def coefficients(case):
    """[Y, Cb, Cr] (block rows, block cols, 64 zig-zag) over the real blocks: what every variant of the case's file holds."""
    return sr.coefficients(build(case), case.quality, *factors(case))


def flat_coefficients(case):
    return ref.flat_coefficients(coefficients(case)).astype(np.int16)


def table_words(case):
    return np.stack(qtables(case)).astype(np.uint16)


def restart_interval(case, variant):
    return {'rst1': 1, 'rstn': RSTN, 'progB': 2}.get(variant, 0)


@functools.lru_cache(maxsize=None)
def written(case, variant):
    """The test writer's file of a variant."""
    hs, vs = factors(case)
    ri = restart_interval(case, variant)
    if variant == 'rstn':
        g = sr.geometry(case.h, case.w, hs, vs)
        assert (g['my'] * g['mx']) % RSTN and g['my'] * g['mx'] > RSTN
    if variant.startswith('prog'):
        return sr.write_progressive(coefficients(case), case.h, case.w, case.quality, hs, vs,
                                    dprog.STANDARD if variant == 'prog' else dprog.SCRIPT_B, ri)
    return sr.write_baseline(coefficients(case), case.h, case.w, case.quality, hs, vs, ri, optimize=variant == 'opt')


@functools.lru_cache(maxsize=None)
def expected(case, s):
    """uint8 (ceil(h / s), ceil(w / s), 3): the restatement's image at scale 1 / s; read-only."""
    y = sr.decode(coefficients(case), qtables(case), case.h, case.w, *factors(case), s)
    y.setflags(write=False)
    return y


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def pixels_held(case, s):
    return case.h * case.w <= PIXELS_UP_TO


Golden = namedtuple('Golden', 'files pixels crcs')


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: case name -> Golden({variant: file}, {scale: Pillow's uint8 pixels} where they are held,
    {scale: CRC32 of Pillow's pixels} for every scale Pillow was asked for)."""
    z = np.load(GOLDEN)
    assert z['names'].tolist() == IDS, 'golden/jpeg_sampling.npz is out of date: run make_jpegsamp_golden.py'
    ends, blob = np.concatenate([[0], z['file_ends']]), z['files'].tobytes()
    crcs, held = z['crcs'], z['pixels']
    out, k, px = {}, 0, 0
    for i, case in enumerate(CASES):
        files = {}
        for variant in case.variants:
            files[variant] = blob[ends[k]:ends[k + 1]]
            k += 1
        pixels, sums = {}, {}
        for j, s in enumerate(SCALES):
            if not askable(case, s):
                continue
            sums[s] = int(crcs[i, j])
            if pixels_held(case, s):
                rows, cols = -(-case.h // s), -(-case.w // s)
                pixels[s] = held[px:px + rows * cols * 3].reshape(rows, cols, 3)
                px += rows * cols * 3
        out[case.name] = Golden(files, pixels, sums)
    assert k + 1 == len(ends) and px == len(held)
    return out


def golden_files():
    """[(case, variant, file)] of the golden file, in its order."""
    g = golden()
    return [(c, v, g[c.name].files[v]) for c in CASES for v in c.variants]


# ---- the host program, in its three forms (jpegsamp_host.cpp) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(form='', sanitize=True):
    """form: '' = geometry and reconstruction, 'RST' = jpegrst_host.cpp, 'PROG' = jpegdprog_host.cpp, with the wide set of factors."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegsamp_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegsamp_host' + form)
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    flags += ['-DJPEGSAMP_' + form] if form else []
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR, '-I', HERE] + flags + [HOST_SOURCE, '-o', out],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


@contextlib.contextmanager
def _program_of(module, form):
    """The sibling's host_results run over this program: its arguments and file formats are the sibling's."""
    saved = module.host_program
    module.host_program = lambda sanitize: host_program(form, sanitize)
    try:
        yield
    finally:
        module.host_program = saved


def stream_of(name, data):
    """A baseline file -> jpegrst_cases.Stream."""
    p = jpegd_ref.header(data)
    return rc.Stream(name, p['h'], p['w'], p['hs'], p['vs'], rref.parse(data)['ri'], jpegd_ref.huffman_bytes(p),
                     data[p['ecd_offset']:len(data) - 2])


@functools.lru_cache(maxsize=None)
def baseline_streams():
    return [stream_of('{}/{}'.format(c.name, v), f) for c, v, f in golden_files() if not v.startswith('prog')]


@functools.lru_cache(maxsize=None)
def progressive_files():
    return [dpc._file('{}/{}'.format(c.name, v), f, flat_coefficients(c)) for c, v, f in golden_files() if v.startswith('prog')]


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """Damage to the baseline golden streams, every choice from a fixed seed: single-bit flips, a truncation, and for the streams with
    markers one renumbered and one removed."""
    rng = np.random.default_rng(20261021)
    out = []
    for s in baseline_streams():
        for j in range(3):
            bit = int(rng.integers(0, 8 * len(s.ecd)))
            ecd = bytearray(s.ecd)
            ecd[bit >> 3] ^= 0x80 >> (bit & 7)
            out.append(s._replace(name='{}|flip{}'.format(s.name, bit), ecd=bytes(ecd)))
        out.append(s._replace(name=s.name + '|cut', ecd=s.ecd[:len(s.ecd) // 2]))
        at = rc._marker_positions(s.ecd)
        if at:
            k = at[int(rng.integers(0, len(at)))]
            out.append(s._replace(name=s.name + '|renumber', ecd=s.ecd[:k + 1] + bytes([0xd0 | ((s.ecd[k + 1] + 3) & 7)]) + s.ecd[k + 2:]))
            out.append(s._replace(name=s.name + '|remove', ecd=s.ecd[:k] + s.ecd[k + 2:]))
    return out


@functools.lru_cache(maxsize=None)
def damaged_progressive():
    """Every scan of every progressive golden file cut in half, and eight single-bit flips per file, from a fixed seed."""
    rng = np.random.default_rng(20261022)
    out = []
    for f in progressive_files():
        for s, seg in enumerate(f.segments):
            segs = list(f.segments)
            segs[s] = seg[:len(seg) // 2]
            out.append(f._replace(name='{}|cut{}'.format(f.name, s), segments=segs, expected=None, data=None))
        for j in range(8):
            s = int(rng.integers(0, len(f.segments)))
            if not f.segments[s]:
                continue
            bit = int(rng.integers(0, 8 * len(f.segments[s])))
            seg = bytearray(f.segments[s])
            seg[bit >> 3] ^= 0x80 >> (bit & 7)
            segs = list(f.segments)
            segs[s] = bytes(seg)
            out.append(f._replace(name='{}|flip{}.{}'.format(f.name, s, bit), segments=segs, expected=None, data=None))
    return out


@functools.lru_cache(maxsize=None)
def host_baseline():
    """The sanitized RST form over the valid and the damaged baseline streams: (streams, results, recoded, completed process)."""
    streams = baseline_streams() + damaged_streams()
    with _program_of(rc, 'RST'):
        return (streams,) + rc.host_results(streams, SETTINGS + (0,))


@functools.lru_cache(maxsize=None)
def host_progressive():
    """The sanitized PROG form over the valid and the damaged progressive files: (files, [Host] or None, completed process)."""
    files = progressive_files() + damaged_progressive()
    with _program_of(dpc, 'PROG'):
        return (files,) + dpc.host_results(files, SETTINGS + (0,))


GEO_FIELDS = ('per', 'ny', 'SB', 'my', 'mx', 'bhY', 'bwY', 'bhC', 'bwC', 'ceh', 'cew', 'nbY', 'nbC', 'NB', 'hsh')
SCALE_FIELDS = ('ok', 'nY', 'nC', 'ehC', 'ewC', 'rx', 'ry', 'mode', 'oh', 'ow')
MODES = {'none': 0, 'replicate': 1, 'h2v1': 2, 'h1v2': 3}           # csrc/jpegscale.h JPEGSCALE_MODE_*


def _run(records, sanitize=True):
    exe = host_program('', sanitize)
    work = tempfile.mkdtemp(prefix='jpegsamp_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(records)) + b''.join(records))
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        blob = open(os.path.join(work, 'out.bin'), 'rb').read() if done.returncode == 0 else b''
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return blob, done


def host_geometry(queries):
    """[(h, w, hs, vs)] -> ([(admitted by the three, admitted by the wide set, {field: value} or None, {scale: {field: value}})], the
    completed process)."""
    blob, done = _run([struct.pack('<6i', 0, h, w, hs, vs, 0) for h, w, hs, vs in queries])
    out, at = [], 0
    if done.returncode == 0:
        for _ in queries:
            three, wide = struct.unpack_from('<2i', blob, at)
            at += 8
            geo, scaled = None, {}
            if wide:
                geo = dict(zip(GEO_FIELDS, struct.unpack_from('<15i', blob, at)))
                at += 60
                for s in REDUCED:
                    scaled[s] = dict(zip(SCALE_FIELDS, struct.unpack_from('<10i', blob, at)))
                    at += 40
            out.append((bool(three), bool(wide), geo, scaled))
        assert at == len(blob)
    return out, done


@functools.lru_cache(maxsize=None)
def host_images():
    """The sanitized program's image of every case at every scale: ({(case name, scale): uint8 image}, the completed process)."""
    jobs = [(c, s) for c in CASES for s in SCALES]
    blob, done = _run([struct.pack('<6i', 1, c.h, c.w, *factors(c), s) + table_words(c).tobytes() + flat_coefficients(c).tobytes()
                       for c, s in jobs])
    out, at = {}, 0
    if done.returncode == 0:
        for c, s in jobs:
            shape = (-(-c.h // s), -(-c.w // s), 3)
            out[(c.name, s)] = np.frombuffer(blob, np.uint8, int(np.prod(shape)), at).reshape(shape)
            at += int(np.prod(shape))
        assert at == len(blob)
    return out, done
