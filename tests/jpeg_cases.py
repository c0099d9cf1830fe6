"""The case list of the baseline JPEG tests (test_jpeg_host.py, test_gpu_jpeg.py, golden/make_jpeg_golden.py) and its builders.
A case is a uint8 batch (n, h, w, 3), a quality and a sub-sampling; the restatement's results are computed once per process."""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np

import jpeg_ref as ref

Case = namedtuple('Case', 'name contents h w quality subsampling golden')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_streams.npz')
QUALITIES = (1, 5, 30, 50, 75, 95, 100)
SUBSAMPLINGS = ('4:4:4', '4:2:2', '4:2:0')


def _image(content, h, w, seed):
    y, x = np.mgrid[:h, :w].astype(np.float64)
    if content == 'noise':
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == 'smooth':
        img = np.stack([128 + 100 * np.sin(x / 7.0) * np.cos(y / 5.0), 255 * x / max(w - 1, 1), 255 * (x + y) / max(h + w - 2, 1)], -1)
    elif content == 'constant':
        img = np.broadcast_to(np.array([200.0, 17.0, 96.0]), (h, w, 3))
    elif content == 'checker':
        img = np.repeat((255 * ((x + y) % 2))[..., None], 3, -1)
    elif content == 'half':
        img = np.repeat((255 * (x >= w // 2))[..., None], 3, -1)
    elif content == 'cosine':
        img = np.repeat((128 + 60 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16))[..., None], 3, -1)
    elif content == 'mixed':              # smooth with a noisy quarter: long and short blocks in one image
        img = _image('smooth', h, w, seed).astype(np.float64)
        img[:h // 2, w // 2:] = _image('noise', h, w, seed)[:h // 2, w // 2:]
    else:
        raise ValueError(content)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _case(contents, h, w, quality, subsampling, golden=True):
    contents = (contents,) if isinstance(contents, str) else tuple(contents)
    name = '{}_{}x{}_q{}_{}'.format('+'.join(contents), h, w, quality, subsampling.replace(':', ''))
    return Case(name, contents, h, w, quality, subsampling, golden)


def _cases():
    out = []
    sizes = ((8, 8), (16, 16), (13, 21), (17, 33), (40, 56))
    for i, (h, w) in enumerate(sizes):
        for j, ss in enumerate(SUBSAMPLINGS):
            k = 3 * i + j
            # every size at every sub-sampling, the qualities in turn; noise fills the golden file, so the two largest sizes carry less
            if (h, w) == (40, 56):
                if ss == '4:2:0':                        # its dummy block row
                    out.append(_case('mixed', h, w, QUALITIES[k % 7], ss))
            elif (h, w) != (17, 33) or ss != '4:4:4':
                out.append(_case('noise', h, w, QUALITIES[k % 7], ss))
            out.append(_case('smooth', h, w, QUALITIES[(k + 3) % 7], ss))
    out.append(_case('noise', 16, 24, 100, '4:4:4'))            # stuffed FF 00 pairs
    for ss in SUBSAMPLINGS:
        out.append(_case('checker', 16, 16, 100, ss))           # AC category 10
        out.append(_case('half', 16, 16, 100, ss))              # DC difference 2040: category 11
        out.append(_case('constant', 16, 16, 75, ss))           # EOB only, DC difference 0
    out.append(_case('constant', 13, 21, 50, '4:2:0'))
    out.append(_case('cosine', 16, 24, 75, '4:4:4'))            # ZRL
    out.append(_case('cosine', 16, 24, 75, '4:2:0'))
    out.append(_case(('noise', 'smooth', 'constant', 'checker'), 16, 24, 75, '4:2:2'))       # a batch whose lengths and padding differ
    out.append(_case(('smooth', 'noise', 'half'), 13, 21, 95, '4:2:0'))
    # beyond the golden file.  Tiny images: one block that is mostly padding; up to two chroma columns libjpeg replicates on decoding
    for (h, w), ss in (((1, 1), '4:2:0'), ((2, 2), '4:2:2'), ((3, 5), '4:2:0'), ((5, 3), '4:2:2'), ((9, 4), '4:2:0'), ((7, 6), '4:4:4')):
        out.append(_case('noise', h, w, 95, ss, golden=False))
    # several workgroups, scans across them
    out.append(_case('noise', 64, 72, 75, '4:2:2', golden=False))
    out.append(_case('smooth', 64, 72, 95, '4:2:0', golden=False))
    out.append(_case('mixed', 64, 72, 1, '4:4:4', golden=False))
    out.append(_case(('mixed', 'smooth'), 128, 192, 75, '4:4:4', golden=False))
    out.append(_case(('noise', 'mixed'), 128, 192, 30, '4:2:0', golden=False))
    out.append(_case('mixed', 256, 256, 75, '4:2:0', golden=False))
    return out


CASES = _cases()
GOLDEN_CASES = [c for c in CASES if c.golden]
IDS = [c.name for c in CASES]


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def build(case):
    """uint8 (n, h, w, 3), read-only."""
    x = np.stack([_image(c, case.h, case.w, zlib.crc32('{}/{}'.format(case.name, i).encode())) for i, c in enumerate(case.contents)])
    x.setflags(write=False)
    return x


Reference = namedtuple('Reference', 'coefs flat files ecds decoded stats')


@functools.lru_cache(maxsize=None)
def reference(case):
    """The restatement's results for a case: per image the coefficients [Y, Cb, Cr], their flat device layout, the whole file, its
    entropy-coded segment, the decoded uint8 image; and the path counters summed over the batch."""
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    stats = {}
    coefs, flat, files, ecds, decoded = [], [], [], [], []
    for img in build(case):
        c = ref.coefficients(img, case.quality, hs, vs)
        ecd = ref.entropy_code(c, case.h, case.w, hs, vs, stats)
        coefs.append(c)
        flat.append(ref.flat_coefficients(c))
        ecds.append(ecd)
        files.append(ref.header(case.h, case.w, case.quality, hs, vs) + ecd + b'\xff\xd9')
        decoded.append(ref.decode_u8(c, case.h, case.w, case.quality, hs, vs))
    return Reference(coefs, np.stack(flat), files, ecds, np.stack(decoded), stats)


@functools.lru_cache(maxsize=None)
def golden():
    """The committed golden file taken apart: case name -> (x uint8 (n,h,w,3), [Pillow's file per image], Pillow's decoded
    uint8 (n,h,w,3))."""
    z = np.load(GOLDEN)
    out, px, pf = {}, 0, 0
    ends = np.concatenate([[0], z['file_ends']])
    blob = z['files'].tobytes()
    for name in z['names'].tolist():
        case = by_name(name)
        n, size = len(case.contents), len(case.contents) * case.h * case.w * 3
        shape = (n, case.h, case.w, 3)
        out[name] = (z['x'][px:px + size].reshape(shape), [blob[ends[pf + i]:ends[pf + i + 1]] for i in range(n)],
                     z['rgb'][px:px + size].reshape(shape))
        px, pf = px + size, pf + n
    return out
