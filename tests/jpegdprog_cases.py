"""The cases of the progressive-JPEG decoder tests (test_jpegdprog_host.py, test_gpu_jpegdprog.py, golden/make_jpegdprog_golden.py):
(a) the Pillow files of jpegprog_cases.golden(), (b) the files of two further scan scripts written by jpegdprog_ref.encode from the
same coefficients, (c) jpegprog_cases' synthetic coefficient tensors coded by the restatement, (d) damaged streams of small cases.
A File is what a decoder needs and what it has to give; host_results() builds tests/jpegdprog_host.cpp and runs it as a process of
its own."""
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

import jpeg_ref as ref
import jpegd_cases
import jpegdprog_ref as dpref
import jpegprog_cases as pc
import jpegprog_ref as pref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpegdprog_streams.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegdprog_host.cpp')
SETTINGS = (32, 64, 256, 2048, 0)            # subsequence bits; 0 = one subsequence per restart interval

# the cases scripts A and B are written for
SCRIPT_CASES = tuple('mixed_37x53_q75_{}_ri{}'.format(ss, ri) for ss in ('444', '422', '420') for ri in (0, 2, 3, 7)) + (
    'mixed_40x56_three_422', 'corr_32x160_q100_420', 'mixed_128x192_q75_420_ri5')

# name: case|image index|script.  data: the whole file, None for a synthetic tensor (it has no header).  expected: flat int16.
File = namedtuple('File', 'name h w hs vs ri script tables segments expected data slow')


def _file(name, data, expected, slow=False):
    p = dpref.split(data)
    return File(name, p['h'], p['w'], p['hs'], p['vs'], p['ri'], tuple(p['script']), [dpref.table_bytes(t) for t in p['tables']],
                p['segments'], expected, data, slow)


def _expected(case):
    return pc.flat(case) if case.slow else pc.reference(case).flat


@functools.lru_cache(maxsize=None)
def golden_files():
    """(a): the 72 files Pillow wrote."""
    out = []
    for name, files in pc.golden().items():
        case = pc.by_name(name)
        for i, data in enumerate(files):
            out.append(_file('{}|{}|std'.format(name, i), data, _expected(case)[i], case.slow))
    return out


def script_file(name, script):
    """The file of script 'A' or 'B' for (the first image of) a case, written by the restatement."""
    case = pc.by_name(name)
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    r = pc.reference(case)
    return dpref.encode(r.coefs[0], case.h, case.w, hs, vs, pref.prefix_of(pc.baseline_header(case)), dpref.SCRIPTS[script], case.ri)


@functools.lru_cache(maxsize=None)
def stored():
    """golden/jpegdprog_streams.npz taken apart: ({'case|script': file}, {file name: CRC32 of the RGB image Pillow decodes from it})."""
    z = np.load(GOLDEN)
    ends = np.concatenate([[0], z['file_ends']])
    blob = z['files'].tobytes()
    files = {n: blob[ends[k]:ends[k + 1]] for k, n in enumerate(z['names'].tolist())}
    return files, dict(zip(z['crc_names'].tolist(), z['crcs'].tolist()))


@functools.lru_cache(maxsize=None)
def script_files():
    """(b): scripts A and B, the stored files (test_jpegdprog_host.py holds the restatement's writer to them)."""
    files = stored()[0]
    return [_file('{}|0|{}'.format(name, s), files['{}|{}'.format(name, s)], pc.reference(pc.by_name(name)).flat[0])
            for s in ('A', 'B') for name in SCRIPT_CASES]


@functools.lru_cache(maxsize=None)
def synthetic_files():
    """(c): the synthetic tensors in libjpeg's script.  What the coder clamps (DC to +-2047, AC to +-1023) is what comes back."""
    out = []
    for s in pc.synthetic():
        _, tables, segs, _ = pc.synthetic_reference(s.name)
        per = []
        for comps, ss, se, ah, al, _, t in pref.SCANS:
            if comps is None:
                per.append(np.stack([tables[0], tables[1], tables[1]]) if ah == 0 else np.zeros((3, 272), np.uint8))
            else:
                per.append(np.stack([tables[t], np.zeros(272, np.uint8), np.zeros(272, np.uint8)]))
        c = s.flat.astype(np.int64).reshape(-1, 64)
        expected = np.clip(c, -1023, 1023)
        expected[:, 0] = np.clip(c[:, 0], -2047, 2047)
        out.append(File(s.name + '|0|std', s.h, s.w, s.hs, s.vs, s.ri, dpref.STANDARD, per, segs, expected.reshape(-1).astype(np.int16),
                        None, False))
    return out


def valid_files(slow=True):
    return [f for f in golden_files() + script_files() + synthetic_files() if slow or not f.slow]


DAMAGE_SOURCES = ('g_smooth_17x33_q95_444|0|std', 'g_noise_13x21_q5_420|0|std', 'mixed_37x53_q75_420_ri2|0|std',
                  'mixed_37x53_q75_422_ri3|0|B', 'mixed_37x53_q75_444_ri0|0|A', 'mixed_37x53_q75_420_ri7|0|B', 'synthetic2_24x40_21_ri3|0|std')


@functools.lru_cache(maxsize=None)
def damaged_files():
    """(d): per source every scan's segment truncated, 40 single-bit flips, random bytes, all FF, a restart marker out of sequence and
    an end-of-band run longer than the scan - every choice from a fixed seed.  expected is None."""
    rng = np.random.default_rng(20241020)
    by = {f.name: f for f in valid_files(False)}
    out = []

    def put(f, tag, s, seg):
        segs = list(f.segments)
        segs[s] = bytes(seg)
        out.append(f._replace(name='{}|{}'.format(f.name, tag), segments=segs, expected=None, data=None))

    for name in DAMAGE_SOURCES:
        f = by[name]
        for s, seg in enumerate(f.segments):
            put(f, 'cut{}.{}'.format(s, len(seg) // 2), s, seg[:len(seg) // 2])
        for j in range(40):
            s = int(rng.integers(0, len(f.segments)))
            bit = int(rng.integers(0, 8 * len(f.segments[s])))
            seg = bytearray(f.segments[s])
            seg[bit >> 3] ^= 0x80 >> (bit & 7)
            put(f, 'flip{}.{}'.format(s, bit), s, seg)
        for j in range(4):
            s = int(rng.integers(0, len(f.segments)))
            put(f, 'random{}.{}'.format(s, j), s, rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes())
        s = int(rng.integers(0, len(f.segments)))
        put(f, 'allff{}'.format(s), s, b'\xff' * 200)
        put(f, 'empty{}'.format(s), s, b'')
        if f.ri:
            for s, seg in enumerate(f.segments):
                at = seg.find(b'\xff\xd0')
                if at >= 0:
                    put(f, 'marker{}'.format(s), s, seg[:at] + b'\xff\xd3' + seg[at + 2:])
        # a run longer than the scan: an AC scan that is nothing but the EOB14 symbol and run bits of all ones
        for s, (cs, ss, se, ah, al) in enumerate(f.script):
            if ss > 0:
                tables = [t.copy() for t in f.tables]
                tables[s] = np.zeros((3, 272), np.uint8)
                tables[s][0, 0], tables[s][0, 16] = 1, 0xe0                  # one code of one bit: EOB14
                seg = bytes([0x7f, 0xfe]) + b'\x00' * 30
                segs = list(f.segments)
                segs[s] = seg
                out.append(f._replace(name='{}|longrun{}'.format(f.name, s), tables=tables, segments=segs, expected=None, data=None))
                break
    return out


# ---- the host program ------------------------------------------------------------------------------------------------------
Host = namedtuple('Host', 'legal levels status rounds coef')       # status, rounds, coef: {setting: value}


@functools.lru_cache(maxsize=None)
def host_program(sanitize):
    """Builds tests/jpegdprog_host.cpp once per process into a temporary directory, removed when the process ends."""
    cxx = jpegd_cases.compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegdprog_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegdprog_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', jpegd_cases.CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


def host_results(files, settings=SETTINGS, sanitize=True):
    """Runs the host program over Files (or anything with h w hs vs ri script tables segments) -> ([Host], the completed process)."""
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegdprog_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(files)))
            for x in files:
                f.write(struct.pack('<6i', x.h, x.w, x.hs, x.vs, x.ri, len(x.script)))
                f.write(dpref_rows(x.script).tobytes())
                for t, seg in zip(x.tables, x.segments):
                    f.write(np.ascontiguousarray(t, np.uint8).tobytes() + struct.pack('<I', len(seg)) + bytes(seg))
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')] + [str(v) for v in settings],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if done.returncode != 0:
            return None, done
        blob = open(os.path.join(work, 'out.bin'), 'rb').read()
        out, at = [], 0
        for x in files:
            n = len(x.script)
            legal, = struct.unpack_from('<i', blob, at)
            at += 4
            if not legal:
                out.append(Host(False, None, {}, {}, {}))
                continue
            levels = list(struct.unpack_from('<{}i'.format(n), blob, at))
            at += 4 * n
            status, rounds, coef = {}, {}, {}
            for v in settings:
                status[v], = struct.unpack_from('<I', blob, at)
                rounds[v] = list(struct.unpack_from('<{}I'.format(n), blob, at + 4))
                ncoef, = struct.unpack_from('<I', blob, at + 4 + 4 * n)
                coef[v] = np.frombuffer(blob, np.int16, ncoef, at + 8 + 4 * n)
                at += 8 + 4 * n + 2 * ncoef
            out.append(Host(True, levels, status, rounds, coef))
        assert at == len(blob)
        return out, done
    finally:
        shutil.rmtree(work, ignore_errors=True)


def dpref_rows(script):
    """A script as the host program and the library take it, the level left 0 where the script is not legal."""
    rows = np.zeros((len(script), 6), np.int32)
    for i, (cs, ss, se, ah, al) in enumerate(script):
        rows[i, :5] = [sum(1 << c for c in set(cs)), ss, se, ah, al]
    if dpref.legal(script):
        rows[:, 5] = dpref.levels(script)
    return rows


def whole_bits(f):
    """A subseq_bits for the library that is at least every scan of the file (the host program's setting 0)."""
    return max(32, -(-8 * max(len(s) for s in f.segments) // 32) * 32)


def crc(rgb):
    return zlib.crc32(np.ascontiguousarray(rgb, np.uint8).tobytes())
