"""The cases of the scaled-decoding tests (test_jpegscale_host.py, test_gpu_jpegscale.py, golden/make_jpegscale_golden.py; DESIGN.md
section 4q).  A case is one uint8 image rebuilt from a seed, a quality, a sampling ('L' = a mode 'L' image, one component) and the
variants of the file the golden file holds for it - Pillow's files:
    plain   baseline, Annex K tables      prog   progressive=True      rst   restart_marker_blocks=2
and for every scale in 1, 2, 4, 8 that Pillow can be asked for the pixels it decodes after draft().  The sizes are the smallest at which
the scaled paths can go wrong: single blocks, ragged edges both ways, the two sides of the width at which libjpeg's 4:2:2 up-sampling
changes from replication to the triangle filter at every scale (a scaled chroma row of 2 | 3 samples: w = 4 s | 4 s + 1), the widths at
1/8 above that threshold where replication must still come out (33, 40, 53, 80), and 136 x 136, whose 289 luma blocks are more than
one 256-thread workgroup.  Every size meets every sampling; qualities and contents go round, and one size carries all of them.  The
restatement's results are computed once per process."""
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
import jpeggrey_ref as gref
import jpegscale_ref as sref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_scaled.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegscale_host.cpp')
SCALES = sref.SCALES
REDUCED = (2, 4, 8)                             # what csrc/jpegscale.h serves: scale 1 is the full-size reconstruction
SAMPLINGS = ('4:4:4', '4:2:2', '4:2:0', 'L')
SIZES = ((8, 8), (16, 16), (17, 9), (5, 3), (9, 33), (24, 17), (33, 32), (37, 53), (64, 40), (48, 80), (16, 8), (16, 9))
QUALITIES = (30, 90, 100)
CONTENTS = ('noise', 'mixed')                   # 'mixed': jpeg_cases' smooth ramps with a quarter of noise
FULL = (24, 17)                                 # the size that carries every quality and content at every sampling
VARIED = (37, 53)                               # the size whose files also come progressive and with restart intervals
BIG = (136, 136)                                # its pixels are held as CRC32 only
RESTART_BLOCKS = 2

Case = namedtuple('Case', 'name content seed h w quality sampling variants')


def _case(content, seed, h, w, quality, sampling, variants=('plain',)):
    name = '{}_{}x{}_q{}_{}'.format(content, h, w, quality, sampling.replace(':', ''))
    return Case(name, content, seed, h, w, quality, sampling, tuple(variants))


def _cases():
    out, k = [], 0
    for h, w in SIZES:
        for sampling in SAMPLINGS:
            if (h, w) == FULL:
                out += [_case(c, 100 + len(out), h, w, q, sampling) for q in QUALITIES for c in CONTENTS]
                continue
            variants = ('plain', 'prog', 'rst') if (h, w) == VARIED else ('plain',)
            out.append(_case(CONTENTS[k % 2], 100 + len(out), h, w, QUALITIES[k % 3], sampling, variants))
            k += 1
        k += 1                                   # the next size starts one further round
    out.append(_case('mixed', 99, BIG[0], BIG[1], 90, '4:2:0'))
    return out


CASES = _cases()
IDS = [c.name for c in CASES]
# sizes Pillow cannot be asked for at 1/8 - a side shorter than the scale: the restatement alone is the expected value
TINY = [_case('noise', 90 + i, h, w, 75, sampling) for i, ((h, w), sampling) in
        enumerate((((1, 1), '4:2:0'), ((3, 5), '4:2:2'), ((5, 3), '4:4:4'), ((3, 5), 'L')))]


def by_name(name):
    return next(c for c in CASES + TINY if c.name == name)


def askable(case, s):
    """Pillow's draft() reaches scale s only by a requested size of at least one pixel a side."""
    return case.h >= s and case.w >= s


def factors(case):
    """(hs, vs) as jpeg_ref takes them; (1, 1) for a one-component case."""
    return (1, 1) if case.sampling == 'L' else ref.SUBSAMPLING[case.sampling]


@functools.lru_cache(maxsize=None)
def build(case):
    """uint8 (h, w, 3), or (h, w) for sampling 'L'; read-only."""
    x = jpeg_cases._image(case.content, case.h, case.w, case.seed)
    x = np.ascontiguousarray(x[..., 0]) if case.sampling == 'L' else x
    x.setflags(write=False)
    return x


def qtables(case):
    """One table per component, natural order."""
    if case.sampling == 'L':
        return [ref.qtable(case.quality, 0)]
    return [ref.qtable(case.quality, 0), ref.qtable(case.quality, 1), ref.qtable(case.quality, 1)]


@functools.lru_cache(maxsize=None)
def coefficients(case):
    """The restatement's coefficients per component, (block rows, block cols, 64 zig-zag) over the real blocks: those of Pillow's file
    (make_jpegscale_golden.py holds the restated file to it)."""
    if case.sampling == 'L':
        return [gref.coefficients(build(case), qtables(case)[0])]
    return ref.coefficients(build(case), case.quality, *factors(case))


def restated_file(case):
    """The restatement's baseline file of the case: Pillow's 'plain' file, byte for byte."""
    if case.sampling == 'L':
        return gref.encode(coefficients(case)[0], case.h, case.w, qtables(case)[0])[0]
    return ref.encode(build(case), case.quality, case.sampling)


@functools.lru_cache(maxsize=None)
def expected(case, s):
    """uint8 (ceil(h / s), ceil(w / s), 3 | 1): the restatement's image at scale 1 / s; read-only."""
    y = sref.decode_scaled(coefficients(case), qtables(case), case.h, case.w, *factors(case), s)
    y.setflags(write=False)
    return y


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def request(case, s):
    """The size (width, height) that make_jpegscale_golden.py asks Pillow's draft() for to reach scale s."""
    return case.w // s, case.h // s


# further draft() requests the golden file records Pillow's choice for: (h, w, requested width, requested height)
DRAFT_REQUESTS = ((64, 40, 5, 5), (64, 40, 30, 30), (64, 40, 40, 64), (64, 40, 41, 64), (37, 53, 13, 9), (37, 53, 14, 9), (37, 53, 6, 5),
                  (37, 53, 7, 4), (136, 136, 17, 17), (136, 136, 18, 17), (136, 136, 1, 1), (16, 9, 3, 3), (16, 9, 4, 8), (5, 3, 1, 1))

Golden = namedtuple('Golden', 'files pixels crcs')


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: (case name -> Golden({variant: Pillow's file}, {scale: Pillow's uint8 pixels
    (rows, cols, 3 | 1)} for the scales held as pixels, {scale: CRC32 of the pixels} for every scale Pillow was asked for),
    draft: int array of rows (h, w, requested width, requested height, the scale Pillow chose))."""
    z = np.load(GOLDEN)
    assert z['names'].tolist() == IDS, 'golden/jpeg_scaled.npz is out of date: run make_jpegscale_golden.py'
    ends, blob = np.concatenate([[0], z['file_ends']]), z['files'].tobytes()
    crcs, held = z['crcs'], z['pixels']
    out, k, px = {}, 0, 0
    for i, case in enumerate(CASES):
        files = {}
        for variant in case.variants:
            files[variant] = blob[ends[k]:ends[k + 1]]
            k += 1
        nc = 1 if case.sampling == 'L' else 3
        pixels, sums = {}, {}
        for j, s in enumerate(SCALES):
            if not askable(case, s):
                continue
            sums[s] = int(crcs[i, j])
            if pixels_held(case, s):
                rows, cols = sref.scaled_size(case.h, case.w, s)
                pixels[s] = held[px:px + rows * cols * nc].reshape(rows, cols, nc)
                px += rows * cols * nc
        out[case.name] = Golden(files, pixels, sums)
    assert k + 1 == len(ends) and px == len(held)
    return out, z['draft']


def pixels_held(case, s):
    """The golden file holds Pillow's pixels of the reduced scales of the small cases; of the full-size images (three quarters of all
    pixels, and what the codec's earlier golden files pin already) and of the big case it holds the CRC32 alone."""
    return s > 1 and (case.h, case.w) != BIG


# ---- the host program ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(sanitize=True):
    """Builds tests/jpegscale_host.cpp once per process into a temporary directory, removed when the process ends."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegscale_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegscale_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


def flat_coefficients(case):
    """int16 (real blocks * 64,): one image in the layout of the device tensor."""
    return ref.flat_coefficients(coefficients(case)).astype(np.int16)


def table_words(case):
    """uint16 (components, 64)."""
    return np.stack(qtables(case)).astype(np.uint16)


Job = namedtuple('Job', 'cases scale')           # a batch: cases of ONE geometry (size and sampling), decoded at one scale


def host_images(jobs, sanitize=True):
    """The host program over `jobs`: ([uint8 (n, rows, cols, 3 | 1) per job], the completed process).
    IN:  uint32 count, then per job int32 n, h, w, hs, vs, nc, scale; n x nc x 64 uint16 tables; n x real blocks x 64 int16 coefficients
    OUT: per job the n images back to back."""
    records = []
    for job in jobs:
        c0 = job.cases[0]
        assert all((c.h, c.w, c.sampling) == (c0.h, c0.w, c0.sampling) for c in job.cases)
        hs, vs = factors(c0)
        rec = struct.pack('<7i', len(job.cases), c0.h, c0.w, hs, vs, len(qtables(c0)), job.scale)
        rec += b''.join(table_words(c).tobytes() for c in job.cases) + b''.join(flat_coefficients(c).tobytes() for c in job.cases)
        records.append(rec)
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegscale_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(records)) + b''.join(records))
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        blob = open(os.path.join(work, 'out.bin'), 'rb').read() if done.returncode == 0 else b''
    finally:
        shutil.rmtree(work, ignore_errors=True)
    images, at = [], 0
    if done.returncode == 0:
        for job in jobs:
            c0 = job.cases[0]
            shape = (len(job.cases),) + sref.scaled_size(c0.h, c0.w, job.scale) + (len(qtables(c0)),)
            size = int(np.prod(shape))
            images.append(np.frombuffer(blob, np.uint8, size, at).reshape(shape))
            at += size
        assert at == len(blob)
    return images, done


def batch_of_five(sampling):
    """Five cases of one geometry (FULL carries six at every sampling): a batch whose image offsets in coefficients, planes and output
    count."""
    return tuple(c for c in CASES if (c.h, c.w) == FULL and c.sampling == sampling)[:5]


@functools.lru_cache(maxsize=None)
def host_jobs():
    """Every case (the tiny ones included) alone at every reduced scale, then a batch of five at every sampling and reduced scale."""
    jobs = [Job((c,), s) for c in CASES + TINY for s in REDUCED]
    jobs += [Job(batch_of_five(sampling), s) for sampling in SAMPLINGS for s in REDUCED]
    return tuple(jobs)


@functools.lru_cache(maxsize=None)
def host_reference():
    """The sanitized host program over host_jobs(), once per process: ({job: images}, the completed process)."""
    images, done = host_images(host_jobs())
    return dict(zip(host_jobs(), images)), done
