"""Writes tests/golden/jpeg_qtab_streams.npz: for every case of tests/jpegq_cases.py the whole file Pillow (libjpeg) writes with the
case's quantisation tables - Image.save(format='JPEG', qtables=[...], subsampling=s) - and the image Pillow decodes from it, and for
one image per table kind and sub-sampling also the optimize=True file.  It pins the writer with caller-given tables to libjpeg on
machines without Pillow.  The inputs are rebuilt by jpegq_cases.image, so no source pixels are stored; tests/jpegq_cases.py golden()
takes the file apart again.
    python tests/golden/make_jpegq_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402
import jpegq_cases  # noqa: E402


def pillow(img, tables, subsampling, optimize=False):
    """uint8 (h, w, 3), (T, 64) tables in natural order -> (the bytes of the file, the uint8 image decoded from it)."""
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, format='JPEG', qtables=[[int(v) for v in t] for t in tables],
                                          subsampling=jpeg_cases.SUBSAMPLINGS.index(subsampling), optimize=optimize)
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def main():
    files, rgb, opt = [], [], []
    for case in jpegq_cases.CASES:
        data, decoded = pillow(jpegq_cases.image(case), jpegq_cases.tables(case.kind), case.subsampling)
        files.append(data)
        rgb.append(decoded.reshape(-1))
    for case in jpegq_cases.OPTIMIZED:
        opt.append(pillow(jpegq_cases.image(case), jpegq_cases.tables(case.kind), case.subsampling, optimize=True)[0])
    np.savez_compressed(jpegq_cases.GOLDEN, names=np.array(jpegq_cases.IDS), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64), rgb=np.concatenate(rgb),
                        opt_names=np.array([c.name for c in jpegq_cases.OPTIMIZED]), opt_files=np.frombuffer(b''.join(opt), np.uint8),
                        opt_ends=np.cumsum([len(f) for f in opt]).astype(np.int64))
    print(jpegq_cases.GOLDEN, os.path.getsize(jpegq_cases.GOLDEN), 'bytes;', len(files), 'files,', len(opt), 'optimised')
    assert os.path.getsize(jpegq_cases.GOLDEN) < 256 * 1024


if __name__ == '__main__':
    main()
