"""The cases of the grey-scale JPEG tests (test_jpeggrey_host.py, test_gpu_jpeggrey.py, golden/make_jpeggrey_golden.py; DESIGN.md
section 4p).  A case is a uint8 batch (n, h, w) of images rebuilt from seeds, a quality or a quantisation table, a restart interval in
blocks and the variants of the file the golden file holds for it - Pillow's files for the mode 'L' image:
    plain   Annex K tables                 opt    optimize=True
    prog    progressive=True (six scans)   s22    subsampling=2: the sole component declares the factors 2x2, the same data bytes
The shapes are the smallest at which the one-component paths can go wrong: one pixel, one block, 3 x 4 blocks ragged both ways, more
blocks than one round of the 1024-thread scans (264 x 264 = 1089), 4096 flat blocks in a progressive file (long end-of-band runs,
refinement scans with nothing to refine).  Beside Pillow's files: one whose tables carry ids other than 0 and one of a second legal
one-component script, both made here.  The restatement's results are computed once per process."""
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
import jpeggrey_ref as gref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_grey_streams.npz')
HOST_SOURCE = os.path.join(HERE, 'jpeggrey_host.cpp')
SETTINGS = (32, 256, 2048, 0)                      # subsequence bits of the host program; 0 = subsequences as long as the stream

Case = namedtuple('Case', 'name contents seeds h w quality qt ri variants')
# quantisation tables in natural order: ones give the longest codes; 'arb' is an arbitrary table with entries up to 255
QTABLES = {'ones': np.ones(64, np.int64), 'arb': np.array([1 + (37 * k * k + 11 * k) % 255 for k in range(64)], np.int64)}


def _case(contents, seeds, h, w, quality=75, qt=None, ri=0, variants=('plain', 'opt')):
    contents = (contents,) if isinstance(contents, str) else tuple(contents)
    seeds = (seeds,) if isinstance(seeds, int) else tuple(seeds)
    name = '{}_{}x{}_{}_ri{}'.format('+'.join(contents), h, w, 'qt-' + qt if qt else 'q{}'.format(quality), ri)
    return Case(name, contents, seeds, h, w, quality, qt, ri, tuple(variants))


BATCH = (('flat', 'noise', 'mixed'), (1, 2, 3))          # different content: the lengths and the padding differ


def _cases():
    out = [_case('noise', 5, 1, 1), _case('noise', 6, 8, 8, quality=100)]
    out.append(_case(*BATCH, 20, 27, variants=('plain', 'opt', 'prog', 's22')))
    out.append(_case(*BATCH, 20, 27, quality=1))
    out.append(_case(*BATCH, 20, 27, quality=50, variants=('plain',)))
    out.append(_case(*BATCH, 20, 27, quality=100))
    out.append(_case(('noise', 'mixed'), (7, 8), 20, 27, qt='ones'))
    out.append(_case(('noise', 'mixed'), (7, 8), 20, 27, qt='arb', variants=('plain',)))
    for ri in (1, 2, 4, 5):                          # one block, two, a block row, one that does not divide the 12 blocks
        out.append(_case(('noise', 'mixed'), (9, 10), 20, 27, ri=ri))
    out.append(_case('mixed', 11, 264, 264))
    out.append(_case('mixed', 11, 264, 264, ri=33, variants=('plain',)))           # a block row; 32 markers: the numbers wrap past D7
    out.append(_case('flat', 12, 512, 512, variants=('prog',)))
    out.append(_case('noise', 13, 64, 64, variants=('plain', 'prog')))
    return out


CASES = _cases()
IDS = [c.name for c in CASES]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def _image(content, h, w, seed):
    """uint8 (h, w): 'flat' one grey level, 'noise' uniform noise, 'mixed' / 'smooth' the first channel of jpeg_cases' natural crops."""
    if content == 'flat':
        return np.full((h, w), 40 + 13 * seed % 160, np.uint8)
    return np.ascontiguousarray(jpeg_cases._image(content, h, w, seed)[..., 0])


@functools.lru_cache(maxsize=None)
def build(case):
    """uint8 (n, h, w), read-only."""
    x = np.stack([_image(c, case.h, case.w, s) for c, s in zip(case.contents, case.seeds)])
    x.setflags(write=False)
    return x


def qtable(case):
    """The one table of a case's files, (64,) int64 in natural order."""
    return QTABLES[case.qt] if case.qt else ref.qtable(case.quality, 0)


@functools.lru_cache(maxsize=None)
def coefficients(case):
    """Per image the restatement's coefficients (block rows, block cols, 64)."""
    return [gref.coefficients(img, qtable(case)) for img in build(case)]


@functools.lru_cache(maxsize=None)
def restated(case, variant):
    """The restatement's files of a case's variant and their Huffman tables ((2, 272); None where the variant has Annex K's or is
    progressive): ([file per image], [tables per image])."""
    qt = qtable(case)
    if variant == 'prog':
        return [gref.encode_progressive(c, case.h, case.w, qt, gref.SCRIPT_STD, case.ri) for c in coefficients(case)], None
    done = [gref.encode(c, case.h, case.w, qt, case.ri, variant == 'opt', 0x22 if variant == 's22' else 0x11) for c in coefficients(case)]
    return [d[0] for d in done], ([d[1] for d in done] if variant == 'opt' else None)


@functools.lru_cache(maxsize=None)
def decoded(case):
    """uint8 (n, h, w): what libjpeg decodes from any variant of the case, by the restatement."""
    return np.stack([gref.decode_u8(c, qtable(case), case.h, case.w) for c in coefficients(case)])


Golden = namedtuple('Golden', 'files pixels')


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: case name -> Golden({variant: [Pillow's file per image]}, Pillow's decoded uint8
    (n, h, w) of the case's first variant)."""
    z = np.load(GOLDEN)
    assert z['names'].tolist() == IDS, 'golden/jpeg_grey_streams.npz is out of date: run make_jpeggrey_golden.py'
    ends, blob = np.concatenate([[0], z['file_ends']]), z['files'].tobytes()
    out, k, px = {}, 0, 0
    for case in CASES:
        n, files = len(case.contents), {}
        for variant in case.variants:
            files[variant] = [blob[ends[k + i]:ends[k + i + 1]] for i in range(n)]
            k += n
        size = n * case.h * case.w
        out[case.name] = Golden(files, z['pixels'][px:px + size].reshape(n, case.h, case.w))
        px += size
    assert k + 1 == len(ends)
    return out


# ---- files made here ---------------------------------------------------------------------------------------------------------------
def other_ids(data, tq=2, td=1, ta=3):
    """A baseline grey-scale file with its tables under other ids: quantisation table `tq`, DC table `td`, AC table `ta` - the DQT and DHT
    segments, the frame's Tq and the scan's selectors renamed, not a bit of the data changed."""
    p = gref.split(data)
    head = bytearray(data[:p['ecd_offset']])
    dqt, sof, sos = head.index(b'\xff\xdb'), head.index(b'\xff\xc0'), head.index(b'\xff\xda')
    dht0 = head.index(b'\xff\xc4')
    dht1 = head.index(b'\xff\xc4', dht0 + 2)
    assert head[dqt + 4] == 0 and head[sof + 12] == 0 and head[dht0 + 4] == 0x00 and head[dht1 + 4] == 0x10 and head[sos + 6] == 0
    head[dqt + 4], head[sof + 12], head[dht0 + 4], head[dht1 + 4], head[sos + 6] = tq, tq, td, 0x10 | ta, (td << 4) | ta
    return bytes(head) + data[p['ecd_offset']:]


@functools.lru_cache(maxsize=None)
def made_here():
    """name -> (file, the case whose images and coefficients it holds, image index): the file with other table ids, and the files of the
    second script (a 3 x 4 block image with its ragged edges, and noise over 64 blocks)."""
    small, noise = by_name('flat+noise+mixed_20x27_q75_ri0'), by_name('noise_64x64_q75_ri0')
    out = {'ids': (other_ids(golden()[small.name].files['opt'][2]), small, 2)}
    for tag, case, i in (('bands20x27', small, 2), ('bands64x64', noise, 0)):
        out[tag] = (gref.encode_progressive(coefficients(case)[i], case.h, case.w, qtable(case), gref.SCRIPT_BANDS), case, i)
    return out


# ---- streams as the host program and nimg_jpeg_grey_decode take them -------------------------------------------------------------------
Stream = namedtuple('Stream', 'name h w ri huffman ecd')         # ri: the DRI value the decoder is given; huffman: (2, 272) uint8


@functools.lru_cache(maxsize=None)
def valid_streams():
    """Every baseline file of the golden file and the one with other ids; named case/variant/image."""
    out = []
    files = [('{}/{}/{}'.format(c.name, v, i), data) for c in CASES for v in c.variants if v != 'prog'
             for i, data in enumerate(golden()[c.name].files[v])] + [('made/ids/0', made_here()['ids'][0])]
    for name, data in files:
        p = gref.split(data)
        out.append(Stream(name, p['h'], p['w'], p['ri'], gref.table_bytes(p['tables'][0]), p['segments'][0]))
    return out


def _marker_positions(ecd):
    return [k for k in range(len(ecd) - 1) if ecd[k] == 0xff and 0xd0 <= ecd[k + 1] <= 0xd7]


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """Damage from a fixed seed.  To every small stream: single-bit flips and a truncation.  To those with markers: a marker renumbered,
    removed or duplicated, and a DRI value that is not the file's."""
    rng = np.random.default_rng(20261020)
    small = [s for s in valid_streams() if s.h <= 64]
    marked = [s for s in small if _marker_positions(s.ecd)]
    out = []

    def add(s, kind, ecd=None, ri=None):
        out.append(s._replace(name='{}|{}'.format(s.name, kind), ecd=s.ecd if ecd is None else bytes(ecd), ri=s.ri if ri is None else ri))

    for j in range(120):
        s = small[j % len(small)]
        bit = int(rng.integers(0, 8 * len(s.ecd)))
        ecd = bytearray(s.ecd)
        ecd[bit >> 3] ^= 0x80 >> (bit & 7)
        add(s, 'flip{}'.format(bit), ecd)
    for j, s in enumerate(small):
        add(s, 'truncate{}'.format(j), s.ecd[:len(s.ecd) - 1 - int(rng.integers(0, max(len(s.ecd) // 2, 1)))])
    for j in range(30):
        s = marked[j % len(marked)]
        at = _marker_positions(s.ecd)
        k = at[int(rng.integers(0, len(at)))]
        add(s, 'renumber{}'.format(j), s.ecd[:k + 1] + bytes([0xd0 | ((s.ecd[k + 1] + int(rng.integers(1, 8))) & 7)]) + s.ecd[k + 2:])
        add(s, 'remove{}'.format(j), s.ecd[:k] + s.ecd[k + 2:])
        add(s, 'duplicate{}'.format(j), s.ecd[:k + 2] + s.ecd[k:])
    for j, s in enumerate(marked[:12]):
        add(s, 'dri+{}'.format(j), ri=s.ri + 1 + j % 3)
    return out


@functools.lru_cache(maxsize=None)
def progressive_files():
    """name -> file: Pillow's progressive files and those of the second script."""
    out = {'{}/prog/{}'.format(c.name, i): data for c in CASES if 'prog' in c.variants for i, data in enumerate(golden()[c.name].files['prog'])}
    out.update({'made/{}/0'.format(tag): v[0] for tag, v in made_here().items() if tag != 'ids'})
    return out


def damaged_progressive():
    """name -> file: a bit flipped in every scan of the small progressive files, and the last scan cut short."""
    rng = np.random.default_rng(20261021)
    out = {}
    for name, data in progressive_files().items():
        p = gref.split(data)
        if p['h'] > 64:
            continue
        at = p['ecd_offset']
        for s, seg in enumerate(p['segments']):
            lo = data.index(seg, at) if seg else at
            at = lo + len(seg)
            if len(seg) > 1:
                bit = int(rng.integers(0, 8 * len(seg)))
                flipped = bytearray(data)
                flipped[lo + (bit >> 3)] ^= 0x80 >> (bit & 7)
                if not (flipped[lo + (bit >> 3)] == 0xff or (bit >> 3 and flipped[lo + (bit >> 3) - 1] == 0xff)):      # no new marker
                    out['{}|flip{}.{}'.format(name, s, bit)] = bytes(flipped)
        out['{}|cut'.format(name)] = data[:len(data) - 2 - max(len(p['segments'][-1]) // 2, 1)].rstrip(b'\xff') + b'\xff\xd9'
    return out


# ---- the host program ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(sanitize):
    """Builds tests/jpeggrey_host.cpp once per process into a temporary directory, removed when the process ends."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpeggrey_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpeggrey_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


Host = namedtuple('Host', 'status rounds subsequences coef')


def _run(mode, records, settings, sanitize):
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpeggrey_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(records)) + b''.join(records))
        done = subprocess.run([exe, mode, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')] + [str(v) for v in settings],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        blob = open(os.path.join(work, 'out.bin'), 'rb').read() if done.returncode == 0 else b''
        return blob, done
    finally:
        shutil.rmtree(work, ignore_errors=True)


def host_results(streams, settings=SETTINGS, sanitize=True):
    """The host program's baseline mode over `streams`: ({(stream index, setting): Host}, [recoded per stream: 1 = the coefficients coded
    again with the stream's tables are its bytes, 0 not, 2 not tried], [histogram (2, 257) of the first setting's coefficients], the
    completed process)."""
    records = [struct.pack('<3iI', s.h, s.w, s.ri, len(s.ecd)) + s.huffman.tobytes() + s.ecd for s in streams]
    blob, done = _run('baseline', records, settings, sanitize)
    results, recoded, hists, at = {}, [], [], 0
    if done.returncode == 0:
        for k in range(len(streams)):
            for v in settings:
                status, rounds, nsub, ncoef = struct.unpack_from('<4I', blob, at)
                results[(k, v)] = Host(status, rounds, nsub, np.frombuffer(blob, np.int16, ncoef, at + 16))
                at += 16 + 2 * ncoef
            recoded.append(struct.unpack_from('<I', blob, at)[0])
            hists.append(np.frombuffer(blob, np.uint32, 2 * 257, at + 4).reshape(2, 257))
            at += 4 + 4 * 2 * 257
        assert at == len(blob)
    return results, recoded, hists, done


def host_progressive(files, settings=SETTINGS, sanitize=True):
    """The host program's progressive mode over whole files (taken apart by jpeggrey_ref.split): ({(file index, setting): Host with
    rounds = [per scan]}, the completed process)."""
    records = []
    for data in files:
        p = gref.split(data)
        rows = np.array([[1, ss, se, ah, al, lv] for (_, ss, se, ah, al), lv in zip(p['script'], gref.dpref.levels(p['script']))], np.int32)
        rec = struct.pack('<4i', p['h'], p['w'], p['ri'], len(rows)) + rows.tobytes()
        for pairs, seg in zip(p['tables'], p['segments']):
            rec += struct.pack('<I', len(seg)) + gref.table_bytes(pairs, 1).tobytes() + seg
        records.append(rec)
    blob, done = _run('progressive', records, settings, sanitize)
    results, at = {}, 0
    if done.returncode == 0:
        for k, data in enumerate(files):
            ns = len(gref.split(data)['script'])
            for v in settings:
                status, ncoef = struct.unpack_from('<2I', blob, at)
                rounds = list(struct.unpack_from('<{}I'.format(ns), blob, at + 8))
                results[(k, v)] = Host(status, rounds, None, np.frombuffer(blob, np.int16, ncoef, at + 8 + 4 * ns))
                at += 8 + 4 * ns + 2 * ncoef
        assert at == len(blob)
    return results, done


@functools.lru_cache(maxsize=None)
def host_reference():
    """The sanitized host program over the valid and the damaged baseline streams, once per process: (streams, results, recoded,
    histograms, completed process)."""
    streams = valid_streams() + damaged_streams()
    return (streams,) + host_results(streams)


@functools.lru_cache(maxsize=None)
def host_progressive_reference():
    """The sanitized host program over the valid and the damaged progressive files, once per process: (names, files, results, completed
    process)."""
    files = dict(progressive_files())
    files.update(damaged_progressive())
    names = list(files)
    return (names, [files[n] for n in names]) + host_progressive([files[n] for n in names])
