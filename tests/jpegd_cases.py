"""The files, damaged streams and helpers of the JPEG decoder tests (test_jpegd_host.py, test_gpu_jpegd.py,
golden/make_jpegd_golden.py).  FOREIGN lists the Pillow files the encoder here cannot write - optimised Huffman tables, custom
quantisation tables - which golden/jpegd_streams.npz holds together with Pillow's decode of each; files() adds every file of
golden/jpeg_streams.npz.  host_results() builds tests/jpegd_host.cpp with a host compiler and runs it as a process of its own."""
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
import jpegd_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpegd_streams.npz')
HOST_SOURCE = os.path.join(HERE, 'jpegd_host.cpp')
CORE_DIR = os.path.join(os.path.dirname(HERE), 'neural-imaging_amd', 'csrc')
SETTINGS = (32, 64, 128, 1024, 0)                  # subsequence bits of the host program; 0 = the whole stream

Foreign = namedtuple('Foreign', 'name content h w subsampling quality optimize qtables')

QTABLES = {
    'high': ([255 - 3 * i for i in range(64)], [min(255, 66 + 3 * i) for i in range(64)]),        # entries up to 255
    'reversed': (ref.LUMA[::-1], ref.CHROMA),
}


def _foreign(content, h, w, subsampling, quality=75, optimize=True, qtables=None):
    name = '{}_{}x{}_{}_{}{}'.format(content, h, w, subsampling.replace(':', ''), 'qt-' + qtables if qtables else 'q{}'.format(quality),
                                     '_opt' if optimize else '')
    return Foreign(name, content, h, w, subsampling, quality, optimize, qtables)


def _foreign_cases():
    out = [_foreign('mixed', 24, 32, '4:4:4', 30), _foreign('smooth', 16, 16, '4:4:4', 75), _foreign('smooth', 13, 21, '4:4:4', 100),
           _foreign('noise', 16, 16, '4:2:2', 30), _foreign('noise', 17, 33, '4:2:2', 75),            # 17x33: a dummy block column
           _foreign('smooth', 16, 24, '4:2:2', 100),
           _foreign('noise', 16, 16, '4:2:0', 30), _foreign('mixed', 40, 56, '4:2:0', 75),            # 40x56: a dummy block row
           _foreign('smooth', 13, 21, '4:2:0', 100),
           _foreign('noise', 16, 24, '4:4:4', 100),                                                     # stuffed FF 00 pairs
           _foreign('half', 16, 16, '4:4:4', 100), _foreign('checker', 16, 16, '4:4:4', 100),          # DC category 11, AC category 10
           _foreign('noise', 3, 5, '4:2:0', 75), _foreign('noise', 1, 1, '4:4:4', 75)]
    for content in ('constant', 'smooth', 'noise', 'mixed'):          # one geometry, very different lengths, each its own tables
        out.append(_foreign(content, 24, 32, '4:2:0', 75))
    for key in ('high', 'reversed'):
        for (h, w), ss, content in (((24, 32), '4:4:4', 'mixed'), ((17, 33), '4:2:2', 'noise'), ((40, 56), '4:2:0', 'mixed')):
            out.append(_foreign(content, h, w, ss, optimize=key == 'reversed', qtables=key))
    return out


FOREIGN = _foreign_cases()
UNEQUAL = ['{}_24x32_420_q75_opt'.format(c) for c in ('constant', 'smooth', 'noise', 'mixed')]


def foreign_image(case):
    return jpeg_cases._image(case.content, case.h, case.w, zlib.crc32(case.name.encode()))


File = namedtuple('File', 'name data rgb')


@functools.lru_cache(maxsize=None)
def foreign_files():
    """The committed golden file taken apart: [File(name, Pillow's file, Pillow's decoded uint8 (h, w, 3))]."""
    z = np.load(GOLDEN)
    ends = np.concatenate([[0], z['file_ends']])
    blob = z['files'].tobytes()
    out, px = [], 0
    for k, name in enumerate(z['names'].tolist()):
        case = next(c for c in FOREIGN if c.name == name)
        size = case.h * case.w * 3
        out.append(File(name, blob[ends[k]:ends[k + 1]], z['rgb'][px:px + size].reshape(case.h, case.w, 3)))
        px += size
    assert [f.name for f in out] == [c.name for c in FOREIGN], 'golden/jpegd_streams.npz is out of date: run make_jpegd_golden.py'
    return out


@functools.lru_cache(maxsize=None)
def files():
    """Every file of both golden files."""
    out = []
    for name, (_, gfiles, grgb) in jpeg_cases.golden().items():
        out += [File('{}/{}'.format(name, i), f, grgb[i]) for i, f in enumerate(gfiles)]
    return out + foreign_files()


def by_name(name):
    return next(f for f in files() if f.name == name)


# ---- streams as the host program and nimg_jpeg_decode take them --------------------------------------------------------
Stream = namedtuple('Stream', 'name h w hs vs huffman ecd')          # huffman: (6, 272) uint8


def stream_of(f):
    p = jpegd_ref.header(f.data)
    return Stream(f.name, p['h'], p['w'], p['hs'], p['vs'], jpegd_ref.huffman_bytes(p), f.data[p['ecd_offset']:p['ecd_end']])


@functools.lru_cache(maxsize=None)
def valid_streams():
    return [stream_of(f) for f in files()]


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """Each golden segment truncated at three places, 200 single-bit flips, 20 streams of random bytes and one of all FF - every
    choice from a fixed seed."""
    rng = np.random.default_rng(20240607)
    valid = valid_streams()
    out = []
    for s in valid:
        for k in sorted({len(s.ecd) // 4, len(s.ecd) // 2, len(s.ecd) - 1}):
            out.append(s._replace(name='{}|cut{}'.format(s.name, k), ecd=s.ecd[:k]))
    for j in range(200):
        s = valid[j % len(valid)]
        bit = int(rng.integers(0, 8 * len(s.ecd)))
        ecd = bytearray(s.ecd)
        ecd[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append(s._replace(name='{}|flip{}'.format(s.name, bit), ecd=bytes(ecd)))
    for j in range(20):
        s = valid[int(rng.integers(0, len(valid)))]
        out.append(s._replace(name='{}|random{}'.format(s.name, j), ecd=rng.integers(0, 256, int(rng.integers(1, 600)), dtype=np.uint8).tobytes()))
    s = stream_of(by_name('mixed_40x56_420_q75_opt'))
    out.append(s._replace(name=s.name + '|allff', ecd=b'\xff' * 300))
    return out


def file_of(stream, original):
    """A damaged stream put back behind the header of the file it came from."""
    p = jpegd_ref.header(original)
    return original[:p['ecd_offset']] + stream.ecd + b'\xff\xd9'


# ---- the host program ------------------------------------------------------------------------------------------------------
Host = namedtuple('Host', 'status rounds subsequences coef')


def compiler():
    for cxx in ('g++', 'clang++', os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++')):
        path = shutil.which(cxx)
        if path:
            return path
    return None


@functools.lru_cache(maxsize=None)
def host_program(sanitize):
    """Builds tests/jpegd_host.cpp once per process into a temporary directory, removed when the process ends; returns the
    program's path."""
    cxx = compiler()
    assert cxx, 'no host C++ compiler found'
    work = tempfile.mkdtemp(prefix='jpegd_host_')
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    out = os.path.join(work, 'jpegd_host')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-O1', '-g'] if sanitize else ['-O2']
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CORE_DIR] + flags + [HOST_SOURCE, '-o', out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


def host_results(streams, settings=SETTINGS, sanitize=False):
    """Runs the host program over `streams`; returns {(stream index, setting): Host} and the completed process."""
    exe = host_program(sanitize)
    work = tempfile.mkdtemp(prefix='jpegd_run_')
    try:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I', len(streams)))
            for s in streams:
                f.write(struct.pack('<4iI', s.h, s.w, s.hs, s.vs, len(s.ecd)) + s.huffman.tobytes() + s.ecd)
        done = subprocess.run([exe, os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')] + [str(v) for v in settings],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        results = {}
        if done.returncode == 0:
            blob = open(os.path.join(work, 'out.bin'), 'rb').read()
            at = 0
            for k in range(len(streams)):
                for v in settings:
                    status, rounds, nsub, ncoef = struct.unpack_from('<4I', blob, at)
                    results[(k, v)] = Host(status, rounds, nsub, np.frombuffer(blob, np.int16, ncoef, at + 16))
                    at += 16 + 2 * ncoef
            assert at == len(blob)
        return results, done
    finally:
        shutil.rmtree(work, ignore_errors=True)


def whole_stream_bits(stream):
    """A subseq_bits for nimg_jpeg_decode that is at least the stream (the host program's setting 0)."""
    return max(32, -(-8 * len(stream.ecd) // 32) * 32)
