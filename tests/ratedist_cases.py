"""The cases of the rate-distortion tests (test_gpu_ratedist.py, test_ratedist_host.py): batches for the per-item JPEG kernels with one
quality per item, and the restatement's (tests/jpeg_ref.py) result for one image at one quality, computed once per process."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import jpeg_cases
import jpeg_ref as ref

# 30 and 49: qualities at which libjpeg's integer tables differ from jpeg_helpers.jpeg_qtable's
ITEM_QUALITIES = (1, 5, 30, 49, 50, 75, 95, 100)
CONTENTS = ('noise', 'smooth', 'mixed', 'checker')

ItemCase = namedtuple('ItemCase', 'name n_src h w subsampling n_items')


def _item_cases():
    out = []
    # dummy blocks on both edges at 4:2:0 | odd sizes at 4:2:2 | whole blocks | one pixel | several workgroups
    for n_src, h, w, ss in ((3, 17, 33, '4:2:0'), (2, 13, 21, '4:2:2'), (4, 16, 24, '4:4:4'), (1, 1, 1, '4:2:0'), (2, 64, 72, '4:2:2')):
        for n_items in sorted({n_src, 3 * n_src, 1}):                # every source once | wrap-around | a single item
            out.append(ItemCase('{}x{}x{}_{}_items{}'.format(n_src, h, w, ss.replace(':', ''), n_items), n_src, h, w, ss, n_items))
    return out


ITEM_CASES = _item_cases()
ITEM_IDS = [c.name for c in ITEM_CASES]


@functools.lru_cache(maxsize=None)
def sources(case):
    """uint8 (n_src, h, w, 3), read-only."""
    x = np.stack([jpeg_cases._image(CONTENTS[i % len(CONTENTS)], case.h, case.w, zlib.crc32('{}x{}/{}'.format(case.h, case.w, i).encode()))
                  for i in range(case.n_src)])
    x.setflags(write=False)
    return x


def qualities(case):
    """One quality per item; neighbouring items differ, and so do the visits of one source image when the items wrap around."""
    start = ITEM_CASES.index(case)
    q = [ITEM_QUALITIES[(start + 3 * j) % len(ITEM_QUALITIES)] for j in range(case.n_items)]
    assert all(a != b for a, b in zip(q, q[1:]))
    return q


Restated = namedtuple('Restated', 'flat ecd file decoded')


@functools.lru_cache(maxsize=None)
def restated(case, src, quality):
    """jpeg_ref's result for source image `src` of a case alone at `quality`."""
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    img = sources(case)[src]
    c = ref.coefficients(img, quality, hs, vs)
    ecd = ref.entropy_code(c, case.h, case.w, hs, vs)
    data, decoded = ref.compress(img, quality, case.subsampling)
    assert data == ref.encode(img, quality, case.subsampling) == ref.header(case.h, case.w, quality, hs, vs) + ecd + b'\xff\xd9'
    return Restated(ref.flat_coefficients(c), ecd, data, ref.to_float(decoded))


def rd_images(h, w):
    """float32 (3, h, w, 3) in [0, 1], k / 255: one image of mixed, one of smooth and one of noisy content."""
    x = np.stack([jpeg_cases._image(c, h, w, 7 + i) for i, c in enumerate(('mixed', 'smooth', 'noise'))])
    return x.astype(np.float32) / np.float32(255)


def match_images():
    """float32 (4, 64, 72, 3): contents whose rate and quality at a given JPEG quality differ widely (the two mixed ones by their seed)."""
    x = np.stack([jpeg_cases._image(c, 64, 72, 11 + i) for i, c in enumerate(('mixed', 'smooth', 'noise', 'mixed'))])
    return x.astype(np.float32) / np.float32(255)


def write_pngs(directory, h=176, w=176):
    """Three PNGs of h x w in `directory` (names a.png, b.png, c.png) -> their pixels as float32 / 255, (3, h, w, 3)."""
    import os
    from PIL import Image
    x = np.stack([jpeg_cases._image(c, h, w, 21 + i) for i, c in enumerate(('mixed', 'smooth', 'noise'))])
    for name, img in zip('abc', x):
        Image.fromarray(img).save(os.path.join(str(directory), name + '.png'))
    return x.astype(np.float32) / np.float32(255)
