"""The cases of the restart-interval tests (test_jpegrst_host.py, test_gpu_jpegrst.py, golden/make_jpegrst_golden.py).  A case is a
uint8 batch (n, h, w, 3) of images with given seeds, a quality, a sub-sampling, a restart interval in MCUs and the variants of the
file the golden file holds for it:
    plain   Annex K tables                       opt     optimize=True
    q2, q3  qtables= with two / three tables     q2opt   both
    base, baseopt   the same image without a restart interval (plain / optimize=True)
The seeds of the cases marked `found` were searched for with the restatement (jpegrst_ref.entropy_code's counters) so that the
list reaches every situation test_jpegrst_host.py counts; the restatement's results are computed once per process."""
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
import jpegd_ref
import jpegq_cases
import jpegrst_ref as rref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_rst_streams.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegrst_host.cpp')
SETTINGS = (32, 256, 2048, 0)                      # subsequence bits of the host program; 0 = subsequences as long as the stream

Case = namedtuple('Case', 'name contents seeds h w quality subsampling ri variants')
QTABLES = {'q2': 'random', 'q3': 'three', 'q2opt': 'random'}            # kinds of jpegq_cases.tables


def _case(contents, seeds, h, w, quality, subsampling, ri, variants=('plain', 'opt'), tag=''):
    name = '{}{}_{}x{}_q{}_{}_ri{}'.format(tag, '+'.join(contents), h, w, quality, subsampling.replace(':', ''), ri)
    return Case(name, tuple(contents), tuple(seeds), h, w, quality, subsampling, ri, tuple(variants))


def _cases():
    out = []
    # 3 x 4 MCUs with dummy blocks at the right and the bottom: one MCU, an interval boundary inside a row, one row, a short last
    # interval, the MCU count, more than it, the largest value
    for ri in (1, 3, 4, 5, 12, 13, 65535):
        variants = ('plain', 'opt', 'q2', 'q3', 'q2opt', 'base', 'baseopt') if ri == 5 else ('plain', 'opt')
        out.append(_case(('mixed', 'noise', 'smooth'), (11, 12, 13), 40, 56, 75, '4:2:0', ri, variants))
    out.append(_case(('noise', 'mixed'), (21, 22), 16, 48, 90, '4:4:4', 1))                    # 11 markers: the numbers wrap past D7
    out.append(_case(('mixed', 'noise'), (31, 32), 24, 40, 50, '4:2:2', 2, ('plain', 'opt', 'q3', 'base')))
    out.append(_case(('noise', 'smooth'), (41, 42), 13, 21, 75, '4:2:0', 1))                   # one partial MCU row and column
    out.append(_case(('smooth', 'noise'), (43, 44), 13, 21, 30, '4:4:4', 2, ('plain', 'opt', 'base')))
    # more than 256 subsequences of 32 bits in one image, interval boundaries inside and on chunk boundaries: Ri = 3 MCU rows
    out.append(_case(('noise', 'mixed'), (51, 52), 128, 128, 95, '4:2:0', 24))
    out += [_case(*args, tag='found_') for args in FOUND]
    return out


# searched for (see the module text): (contents, seeds, h, w, quality, sub-sampling, ri).  Noise did not give a data FF as the last
# byte of an interval in 250 000 markers; flat blocks with a checkerboard of their own (a large last coefficient) do within a thousand
# images.
FOUND = (
    (('blocks', 'blocks'), (840, 1060), 8, 64, 100, '4:4:4', 1),
)

CASES = _cases()
IDS = [c.name for c in CASES]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def _image(content, h, w, seed):
    """jpeg_cases' contents, and 'blocks': every 8 x 8 block a flat colour plus a one-pixel checkerboard of its own amplitude per
    channel - its last zig-zag coefficient is large."""
    if content != 'blocks':
        return jpeg_cases._image(content, h, w, seed)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    by, bx = -(-h // 8), -(-w // 8)
    base = rng.integers(0, 256, (by, bx, 3))
    amp = rng.integers(-127, 128, (by, bx, 3))
    sign = (1 - 2 * ((x + y) & 1))[..., None]
    return np.clip(base[y // 8, x // 8] + amp[y // 8, x // 8] * sign, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def build(case):
    """uint8 (n, h, w, 3), read-only."""
    x = np.stack([_image(c, case.h, case.w, s) for c, s in zip(case.contents, case.seeds)])
    x.setflags(write=False)
    return x


def variant_settings(case, variant):
    """(restart interval, optimize, quantisation tables (T, 64) or None) of one variant of a case."""
    ri = 0 if variant.startswith('base') else case.ri
    qt = jpegq_cases.tables(QTABLES[variant]) if variant in QTABLES else None
    return ri, variant.endswith('opt'), qt


@functools.lru_cache(maxsize=None)
def coefficients(case, variant='plain'):
    """Per image the restatement's coefficients [Y, Cb, Cr] with the quantisation of `variant`."""
    import jpegq_ref as qref
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    qt = variant_settings(case, variant)[2]
    return [ref.coefficients(img, case.quality, hs, vs) if qt is None else qref.coefficients(img, qt, hs, vs) for img in build(case)]


Restated = namedtuple('Restated', 'files huffman stats')


@functools.lru_cache(maxsize=None)
def restated(case, variant='plain'):
    """The restatement's files of a case's variant, their Huffman tables (None without optimize) and the situation counters."""
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    ri, optimize, qt = variant_settings(case, variant)
    tables = rref.quality_tables(case.quality) if qt is None else qt
    stats = {}
    done = [rref.encode(c, case.h, case.w, tables, hs, vs, ri, optimize, stats) for c in coefficients(case, variant)]
    return Restated([d[0] for d in done], [d[1] for d in done], stats)


Golden = namedtuple('Golden', 'files rgb')


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: case name -> Golden({variant: [Pillow's file per image]}, Pillow's decoded uint8
    (n, h, w, 3) of the plain files)."""
    z = np.load(GOLDEN)
    assert z['names'].tolist() == IDS, 'golden/jpeg_rst_streams.npz is out of date: run make_jpegrst_golden.py'
    ends, blob = np.concatenate([[0], z['file_ends']]), z['files'].tobytes()
    out, k, px = {}, 0, 0
    for case in CASES:
        n, files = len(case.contents), {}
        for variant in case.variants:
            files[variant] = [blob[ends[k + i]:ends[k + i + 1]] for i in range(n)]
            k += n
        size = n * case.h * case.w * 3
        out[case.name] = Golden(files, z['rgb'][px:px + size].reshape(n, case.h, case.w, 3))
        px += size
    assert k + 1 == len(ends)
    return out


# ---- streams as the host program and nimg_jpeg_decode_restart take them -------------------------------------------------------
Stream = namedtuple('Stream', 'name h w hs vs ri huffman ecd')        # ri: the DRI value the decoder is given; huffman: (6, 272) uint8


@functools.lru_cache(maxsize=None)
def valid_streams():
    """Every file of the golden file, the ones without a restart interval included; named case/variant/image."""
    out = []
    for case in CASES:
        for variant in case.variants:
            for i, data in enumerate(golden()[case.name].files[variant]):
                p = jpegd_ref.header(data)
                out.append(Stream('{}/{}/{}'.format(case.name, variant, i), p['h'], p['w'], p['hs'], p['vs'], rref.parse(data)['ri'],
                                  jpegd_ref.huffman_bytes(p), data[p['ecd_offset']:len(data) - 2]))
    return out


def _marker_positions(ecd):
    return [k for k in range(len(ecd) - 1) if ecd[k] == 0xff and 0xd0 <= ecd[k + 1] <= 0xd7]


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """Damage to the golden streams that carry markers, every choice from a fixed seed: a marker renumbered, removed or duplicated; an
    interval truncated; single-bit flips; random bytes put in front of a marker; a DRI value larger or smaller than the true one."""
    rng = np.random.default_rng(20250611)
    marked = [s for s in valid_streams() if _marker_positions(s.ecd)]
    out = []

    def add(s, kind, ecd=None, ri=None):
        out.append(s._replace(name='{}|{}'.format(s.name, kind), ecd=s.ecd if ecd is None else bytes(ecd), ri=s.ri if ri is None else ri))

    for j in range(40):
        s = marked[j % len(marked)]
        at = _marker_positions(s.ecd)
        k = at[int(rng.integers(0, len(at)))]
        add(s, 'renumber{}'.format(j), s.ecd[:k + 1] + bytes([0xd0 | ((s.ecd[k + 1] + int(rng.integers(1, 8))) & 7)]) + s.ecd[k + 2:])
        add(s, 'remove{}'.format(j), s.ecd[:k] + s.ecd[k + 2:])
        add(s, 'duplicate{}'.format(j), s.ecd[:k + 2] + s.ecd[k:])
        cut = int(rng.integers(1, 12))
        add(s, 'truncate{}'.format(j), s.ecd[:max(k - cut, 0)] + s.ecd[k:])
        stray = bytes(b for b in rng.integers(0, 255, int(rng.integers(1, 9))).tolist())          # (no FF: stray data, no marker)
        add(s, 'stray{}'.format(j), s.ecd[:k] + stray + s.ecd[k:])
    for j in range(120):
        s = marked[j % len(marked)]
        bit = int(rng.integers(0, 8 * len(s.ecd)))
        ecd = bytearray(s.ecd)
        ecd[bit >> 3] ^= 0x80 >> (bit & 7)
        add(s, 'flip{}'.format(bit), ecd)
    for j, s in enumerate(marked[:24]):
        add(s, 'dri+{}'.format(j), ri=s.ri + 1 + j % 3)
        if s.ri > 1:
            add(s, 'dri-{}'.format(j), ri=s.ri - 1)
    for j, s in enumerate(marked[:6]):                       # markers in a stream decoded without an interval: markers like any other
        add(s, 'dri0-{}'.format(j), ri=0)
    return out


@functools.lru_cache(maxsize=None)
def host_program(sanitize):
    """Builds tests/jpegrst_host.cpp once per process into a temporary directory, removed when the process ends."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegrst_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegrst_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


Host = namedtuple('Host', 'status rounds subsequences coef')


def host_results(streams, settings=SETTINGS, sanitize=True):
    """Runs the host program over `streams`: ({(stream index, setting): Host}, [recoded per stream: 1 the same bytes, 0 not, 2 not
    tried], the completed process)."""
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegrst_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(streams)))
            for s in streams:
                f.write(struct.pack('<5iI', s.h, s.w, s.hs, s.vs, s.ri, len(s.ecd)) + s.huffman.tobytes() + s.ecd)
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')] + [str(v) for v in settings],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        results, recoded = {}, []
        if done.returncode == 0:
            blob = open(os.path.join(work, 'out.bin'), 'rb').read()
            at = 0
            for k in range(len(streams)):
                for v in settings:
                    status, rounds, nsub, ncoef = struct.unpack_from('<4I', blob, at)
                    results[(k, v)] = Host(status, rounds, nsub, np.frombuffer(blob, np.int16, ncoef, at + 16))
                    at += 16 + 2 * ncoef
                recoded.append(struct.unpack_from('<I', blob, at)[0])
                at += 4
            assert at == len(blob)
        return results, recoded, done
    finally:
        shutil.rmtree(work, ignore_errors=True)


@functools.lru_cache(maxsize=None)
def host_reference():
    """The sanitized host program's results over the valid and the damaged streams, run once per process: (streams, results,
    recoded, completed process)."""
    streams = valid_streams() + damaged_streams()
    return (streams,) + host_results(streams)
