"""The cases of the tests of the lossless transforms (test_jpegxform_host.py, test_gpu_jpegxform.py, golden/make_jpegxform_golden.py;
DESIGN.md section 4s).  Two kinds.

JOBS - coefficient tensors: every sampling (the eight and grey-scale) x every size x every operation, with edge='trim', and crops at the
origin, in the interior and reaching a ragged edge.  The sizes are the smallest that can go wrong: one block (8 x 8), one MCU of the
sampling, one block row and one block column (8 x 40, 40 x 8), odd chroma block counts (24 x 40: 3 x 5 luma blocks), non-square
(64 x 96), ragged (33 x 50, 17 x 9 - which some operations trim to nothing).  A tensor is random int16 with -32768 and 32767 among
its values, every block stamped with its own index in the DC, which no operation negates: a misplaced block is visible.

FILES - source files and what is made of them: Pillow's 4:4:4, 4:2:2, 4:2:0 and 'L' files - some progressive, some with restart intervals
- and the wide samplings from jpegsamp_ref's writer; per (file, operation, edge, crop) the golden file holds the restatement's output
file, Pillow's decode of it and the size and sampling factors Pillow reports.  Nothing is larger than 96 x 96."""
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
import jpegd_cases
import jpegsamp_ref as sr
import jpegxform_ref as xr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_lossless.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegxform_host.cpp')
OPS = xr.OPS
SAMPLINGS = dict(sr.SAMPLINGS, grey=xr.GREY)             # name -> (hs, vs); grey-scale is (0, 0), as ops.JPEG_GREY
SIZES = ((8, 8), (8, 40), (40, 8), (24, 40), (64, 96), (33, 50), (17, 9))          # (h, w)
PIXELS_UP_TO = 1700                                      # Pillow's pixels are held for output images up to so many pixels, the CRC32 always

# ---- coefficient jobs -------------------------------------------------------------------------------------------------------------------
Job = namedtuple('Job', 'name sampling h w op edge crop n seed')


def factors(sampling):
    return SAMPLINGS[sampling]


def _crops(h, w, hs, vs):
    """At the origin, in the interior, reaching the (ragged) right and bottom edge."""
    mh, mw = xr.imcu(hs, vs)
    out = [(0, 0, min(w, mw + 3), min(h, mh + 5))]
    if w > mw and h > mh:
        out += [(mw, mh, min(w - mw, mw + 1), min(h - mh, 2 * mh)), (mw, mh, w - mw, h - mh)]
    return list(dict.fromkeys(out))


def _jobs():
    out = []
    for sampling, (hs, vs) in SAMPLINGS.items():
        mh, mw = xr.imcu(hs, vs)
        for h, w in list(dict.fromkeys(SIZES + ((mh, mw),))):
            for op in OPS:
                out.append((sampling, h, w, op, 'trim', None, 3 if (h, w) in ((24, 40), (33, 50)) else 1))
        for h, w in ((64, 96), (33, 50)):
            for crop in _crops(h, w, hs, vs):
                for op in OPS:
                    out.append((sampling, h, w, op, 'trim', crop, 1))
    return [Job('{}_{}x{}_{}_{}{}_n{}'.format(s.replace(':', ''), h, w, op, edge, '' if crop is None else '_crop{}.{}.{}.{}'.format(*crop), n),
                s, h, w, op, edge, crop, n, 7000 + k) for k, (s, h, w, op, edge, crop, n) in enumerate(out)]


JOBS = _jobs()
JOB_IDS = [j.name for j in JOBS]
assert len(set(JOB_IDS)) == len(JOB_IDS)


def job_size(job):
    """(h', w', hs', vs') or None where the restatement refuses the job (17 x 9 trimmed to nothing)."""
    try:
        return xr.size(job.h, job.w, *factors(job.sampling), job.op, job.crop, job.edge)
    except ValueError:
        return None


@functools.lru_cache(maxsize=None)
def job_tensor(job):
    """(n, source blocks, 64) int16; read-only."""
    nb = sum(r * c for r, c in xr.shapes(job.h, job.w, *factors(job.sampling)))
    rng = np.random.default_rng(job.seed)
    t = rng.integers(-32768, 32768, (job.n, nb, 64)).astype(np.int16)
    t[rng.random(t.shape) < 0.05] = -32768
    t[rng.random(t.shape) < 0.05] = 32767
    t[..., 0] = (np.arange(job.n * nb).reshape(job.n, nb) * 7 + 1) % 32749                # the stamp
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def job_expected(job):
    """The restatement's (n, output blocks, 64) int16, or None where it refuses."""
    if job_size(job) is None:
        return None
    hs, vs = factors(job.sampling)
    return np.stack([xr.flat(xr.transform(xr.unflat(img.reshape(-1), job.h, job.w, hs, vs), job.h, job.w, hs, vs, job.op, job.crop, job.edge)[0])
                     .reshape(-1, 64) for img in job_tensor(job)])


# ---- the host program (jpegxform_host.cpp) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(sanitize=True):
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegxform_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegxform_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR, '-I', HERE] + flags + [HOST_SOURCE, '-o', out],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


REASONS = {0: 'ok', 1: 'op', 2: 'geometry', 3: 'crop align', 4: 'crop outside', 5: 'partial width', 6: 'partial height', 7: 'empty'}
Query = namedtuple('Query', 'h w hs vs op crop edge')          # (hs, vs) as a caller names them: (0, 0) for grey-scale


def _record(kind, n, q, values=b''):
    hs, vs = q.hs, q.vs
    nc = 1 if (hs, vs) == xr.GREY else 3
    hs, vs = (1, 1) if nc == 1 else (hs, vs)
    op = q.op if isinstance(q.op, int) else OPS.index(q.op)
    crop = (0, 0, 0, 0) if q.crop is None else tuple(q.crop)
    return struct.pack('<14i', kind, n, q.h, q.w, hs, vs, nc, op, *crop, int(q.edge == 'trim'), len(values) // 2) + values


def _run(records, sanitize=True):
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegxform_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(records)) + b''.join(records))
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        blob = open(os.path.join(work, 'out.bin'), 'rb').read() if done.returncode == 0 else b''
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return blob, done


def host_geometry(queries):
    """[Query] -> ([(reason name, (h', w', hs', vs', blocks) or None)], the completed process)."""
    blob, done = _run([_record(0, 1, q) for q in queries])
    out, at = [], 0
    if done.returncode == 0:
        for _ in queries:
            reason, = struct.unpack_from('<i', blob, at)
            at += 4
            geo = None
            if reason == 0:
                geo = struct.unpack_from('<5i', blob, at)
                at += 20
            out.append((REASONS[reason], geo))
        assert at == len(blob)
    return out, done


@functools.lru_cache(maxsize=None)
def host_jobs():
    """The sanitized program over every job: ({job name: ((h', w', hs', vs'), (n, blocks, 64) int16) or None where refused}, the completed
    process).  Built and run once per process."""
    blob, done = _run([_record(1, j.n, Query(j.h, j.w, *factors(j.sampling), j.op, j.crop, j.edge), job_tensor(j).tobytes()) for j in JOBS])
    out, at = {}, 0
    if done.returncode == 0:
        for j in JOBS:
            reason, = struct.unpack_from('<i', blob, at)
            at += 4
            out[j.name] = None
            if reason == 0:
                h, w, hs, vs, nb = struct.unpack_from('<5i', blob, at)
                at += 20
                count = j.n * nb * 64
                out[j.name] = ((h, w) + (xr.GREY if factors(j.sampling) == xr.GREY else (hs, vs)),
                               np.frombuffer(blob, np.int16, count, at).reshape(j.n, nb, 64))
                at += 2 * count
        assert at == len(blob)
    return out, done


# ---- files ------------------------------------------------------------------------------------------------------------------------------
# a source file: who writes it ('pillow' | 'writer' = jpegsamp_ref's), its image, sampling and variant - 'plain', 'opt', 'prog' or 'rstK'
Source = namedtuple('Source', 'name maker content seed h w quality sampling variant')
SOURCES = (
    Source('p444_8x8', 'pillow', 'mixed', 1, 8, 8, 75, '4:4:4', 'plain'),                    # one block
    Source('p420_16x16', 'pillow', 'mixed', 2, 16, 16, 75, '4:2:0', 'opt'),                  # one MCU
    Source('p422_24x40_prog', 'pillow', 'mixed', 3, 24, 40, 50, '4:2:2', 'prog'),            # -> 4:4:0 when transposed
    Source('p420_24x40_rst2', 'pillow', 'mixed', 4, 24, 40, 50, '4:2:0', 'rst2'),            # odd chroma block counts
    Source('p420_64x96', 'pillow', 'mixed', 5, 64, 96, 50, '4:2:0', 'plain'),                # non-square
    Source('p444_33x50_opt', 'pillow', 'mixed', 6, 33, 50, 50, '4:4:4', 'opt'),              # ragged
    Source('p420_17x9', 'pillow', 'noise', 7, 17, 9, 30, '4:2:0', 'plain'),                  # ragged; narrower than an MCU
    Source('grey_8x40', 'pillow', 'mixed', 8, 8, 40, 75, 'grey', 'plain'),                   # one block row
    Source('grey_40x8_prog', 'pillow', 'mixed', 9, 40, 8, 75, 'grey', 'prog'),               # one block column
    Source('grey_33x50_rst3', 'pillow', 'mixed', 10, 33, 50, 50, 'grey', 'rst3'),
    Source('w410_16x32', 'writer', 'mixed', 11, 16, 32, 75, '4:1:0', 'plain'),               # one MCU of 4:1:0 -> 2x4
    Source('w440_24x40', 'writer', 'mixed', 12, 24, 40, 50, '4:4:0', 'opt'),
    Source('w411_33x50_rst2', 'writer', 'mixed', 13, 33, 50, 50, '4:1:1', 'rst2'),           # -> 1x4
    Source('w1x4_64x96', 'writer', 'mixed', 14, 64, 96, 30, '1x4', 'plain'),
    Source('w2x4_40x24', 'writer', 'mixed', 15, 40, 24, 50, '2x4', 'plain'),
)
FileCase = namedtuple('FileCase', 'name source op edge crop')


def _file_cases():
    out = []
    for s in SOURCES:
        hs, vs = factors(s.sampling)
        for op in OPS:
            out.append((s, op, 'trim', None))
        if (s.h, s.w) in ((64, 96), (33, 50)):
            for crop in _crops(s.h, s.w, hs, vs):
                for op in ('none', 'hflip', 'rot90'):
                    out.append((s, op, 'trim', crop))
    return [FileCase('{}|{}|{}{}'.format(s.name, op, edge, '' if crop is None else '|crop{}.{}.{}.{}'.format(*crop)), s, op, edge, crop)
            for s, op, edge, crop in out]


FILE_CASES = _file_cases()
FILE_IDS = [c.name for c in FILE_CASES]
assert len(set(FILE_IDS)) == len(FILE_IDS)


def source_by_name(name):
    return next(s for s in SOURCES if s.name == name)


def restart_interval(source):
    return int(source.variant[3:]) if source.variant.startswith('rst') else 0


def source_image(source):
    x = jpeg_cases._image(source.content, source.h, source.w, source.seed)
    return x[..., 1] if source.sampling == 'grey' else x


def make_source(source):
    """The source file: Pillow's (the golden generator alone calls this for them) or the test writer's."""
    x, ri = source_image(source), restart_interval(source)
    if source.maker == 'writer':
        hs, vs = factors(source.sampling)
        coefs = sr.coefficients(x, source.quality, hs, vs)
        return sr.write_baseline(coefs, source.h, source.w, source.quality, hs, vs, ri, optimize=source.variant == 'opt')
    import io
    from PIL import Image
    buf = io.BytesIO()
    keys = dict(quality=source.quality, optimize=source.variant == 'opt', progressive=source.variant == 'prog')
    if source.sampling != 'grey':
        keys['subsampling'] = source.sampling
    if ri:
        keys['restart_marker_blocks'] = ri
    Image.fromarray(x).save(buf, 'JPEG', **keys)
    return buf.getvalue()


def expected_size(case):
    """(h', w', hs', vs') or None where the case is refused (trimmed to nothing)."""
    s = case.source
    try:
        return xr.size(s.h, s.w, *factors(s.sampling), case.op, case.crop, case.edge)
    except ValueError:
        return None


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


Made = namedtuple('Made', 'data size layer pixels crc')          # the output file; Pillow's Image.size, .layer, pixels (or None) and their CRC32


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: ({source name: file}, {case name: Made, or None where the case is refused})."""
    z = np.load(GOLDEN)
    assert z['sources'].tolist() == [s.name for s in SOURCES] and z['cases'].tolist() == FILE_IDS, \
        'golden/jpeg_lossless.npz is out of date: run make_jpegxform_golden.py'
    ends, blob = np.concatenate([[0], z['source_ends']]), z['source_files'].tobytes()
    sources = {s.name: blob[ends[k]:ends[k + 1]] for k, s in enumerate(SOURCES)}
    ends, blob, held, px = np.concatenate([[0], z['file_ends']]), z['files'].tobytes(), z['pixels'], 0
    made = {}
    for k, case in enumerate(FILE_CASES):
        data = blob[ends[k]:ends[k + 1]]
        if not data:
            made[case.name] = None
            continue
        w, h, nc = (int(v) for v in z['sizes'][k])
        pixels = None
        if h * w <= PIXELS_UP_TO:
            pixels = held[px:px + h * w * nc].reshape((h, w, nc) if nc == 3 else (h, w))
            px += h * w * nc
        made[case.name] = Made(data, (w, h), [tuple(int(v) for v in row) for row in z['layers'][k][:nc]], pixels, int(z['crcs'][k]))
    assert px == len(held)
    return sources, made
