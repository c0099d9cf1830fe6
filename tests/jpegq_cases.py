"""The cases of the quantisation-table tests (test_jpegq_host.py, test_gpu_jpegq.py, golden/make_jpegq_golden.py): five kinds of
table sets, each at the three sub-samplings over four images.  A case is one uint8 image and one table set; the images are rebuilt
from jpeg_cases._image, the restatement's results are computed once per process."""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np

import jpeg_cases
import jpeg_ref as ref
import jpegq_ref as qref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_qtab_streams.npz')
KINDS = ('ones', 'max', 'random', 'three', 'learned')
# one pixel | odd, smooth | a dummy block column at 4:2:2 and 4:2:0 | a dummy block row at 4:2:0
IMAGES = (('noise', 1, 1), ('smooth', 13, 21), ('noise', 17, 33), ('mixed', 40, 56))
OPTIMIZED_IMAGE = ('mixed', 40, 56)        # the image whose optimize=True file the golden file also holds, per kind and sub-sampling

# the float-to-table rule's named inputs: (value, entry, status bits) - ties go to even, 0.5 comes out as 1 through the clamp
RULE = ((0.5, 1, 1), (2.5, 2, 0), (3.5, 4, 0), (0.4, 1, 1), (-3.0, 1, 1), (255.5, 255, 2), (300.0, 255, 2), (float('nan'), 1, 4),
        (float('inf'), 255, 4), (float('-inf'), 1, 4), (1.0, 1, 0), (255.0, 255, 0), (254.5, 254, 0), (1.5, 2, 0))

Case = namedtuple('Case', 'name kind content h w subsampling')


@functools.lru_cache(maxsize=None)
def tables(kind):
    """(T, 64) uint16 in natural order, read-only."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    if kind == 'ones':
        t = np.ones((2, 64))
    elif kind == 'max':
        t = np.full((2, 64), 255)
    elif kind == 'random':
        t = rng.integers(1, 256, (2, 64))
    elif kind == 'three':                      # three distinct tables: Cr has its own
        t = rng.integers(1, 256, (3, 64))
    elif kind == 'learned':                    # what training leaves: a scaled Annex K pair, perturbed, through the float rule
        t = np.clip(np.rint(0.37 * np.array([ref.LUMA, ref.CHROMA], np.float64) + rng.normal(0, 2, (2, 64))), 1, 255)
    else:
        raise ValueError(kind)
    t = t.astype(np.uint16)
    t.setflags(write=False)
    return t


def _cases():
    out = []
    for kind in KINDS:
        for ss in jpeg_cases.SUBSAMPLINGS:
            for content, h, w in IMAGES:
                out.append(Case('{}_{}_{}x{}_{}'.format(kind, content, h, w, ss.replace(':', '')), kind, content, h, w, ss))
    return out


CASES = _cases()
IDS = [c.name for c in CASES]
OPTIMIZED = [c for c in CASES if (c.content, c.h, c.w) == OPTIMIZED_IMAGE]


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def image(case):
    """uint8 (h, w, 3), read-only: the same pixels for every kind and sub-sampling."""
    x = jpeg_cases._image(case.content, case.h, case.w, zlib.crc32('jpegq/{}x{}'.format(case.h, case.w).encode()))
    x.setflags(write=False)
    return x


Restated = namedtuple('Restated', 'file decoded flat')


@functools.lru_cache(maxsize=None)
def restated(case, optimize=False):
    return Restated(*qref.compress(image(case), tables(case.kind), case.subsampling, optimize))


Golden = namedtuple('Golden', 'file rgb optimized')


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: case name -> Golden(Pillow's file, Pillow's decoded uint8 (h, w, 3), Pillow's
    optimize=True file or None)."""
    z = np.load(GOLDEN)
    names = z['names'].tolist()
    assert names == IDS, 'golden/jpeg_qtab_streams.npz is out of date: run make_jpegq_golden.py'
    ends, blob = np.concatenate([[0], z['file_ends']]), z['files'].tobytes()
    oends, oblob = np.concatenate([[0], z['opt_ends']]), z['opt_files'].tobytes()
    onames = z['opt_names'].tolist()
    out, px = {}, 0
    for k, name in enumerate(names):
        case = by_name(name)
        size = case.h * case.w * 3
        j = onames.index(name) if name in onames else None
        out[name] = Golden(blob[ends[k]:ends[k + 1]], z['rgb'][px:px + size].reshape(case.h, case.w, 3),
                           None if j is None else oblob[oends[j]:oends[j + 1]])
        px += size
    return out
