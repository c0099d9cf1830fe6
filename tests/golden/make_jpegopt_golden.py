"""Writes tests/golden/jpeg_opt_streams.npz: for every golden case of tests/jpeg_cases.py the whole file Pillow (libjpeg) writes for
each image with optimize=True - per-image Huffman tables.  It pins the optimised-Huffman writer to libjpeg on machines without
Pillow.  The inputs are rebuilt by jpeg_cases.build, so no pixels are stored: one byte vector of all files in case order, the file
ends and the case names; tests/jpegopt_cases.py golden() takes them apart again.
    python tests/golden/make_jpegopt_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402
import jpegopt_cases  # noqa: E402


def pillow(img, quality, subsampling):
    """uint8 (h, w, 3) -> the bytes of the file with optimised Huffman tables."""
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling=jpeg_cases.SUBSAMPLINGS.index(subsampling), optimize=True)
    return buf.getvalue()


def main():
    names, files = [], []
    for case in jpeg_cases.GOLDEN_CASES:
        names.append(case.name)
        files += [pillow(img, case.quality, case.subsampling) for img in jpeg_cases.build(case)]
    np.savez_compressed(jpegopt_cases.GOLDEN, names=np.array(names), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64))
    print(jpegopt_cases.GOLDEN, os.path.getsize(jpegopt_cases.GOLDEN), 'bytes;', len(names), 'cases,', len(files), 'files')


if __name__ == '__main__':
    main()
