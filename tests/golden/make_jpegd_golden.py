"""Writes tests/golden/jpegd_streams.npz: the Pillow (libjpeg) files of tests/jpegd_cases.py FOREIGN - optimised Huffman tables,
custom quantisation tables: files the encoder here cannot write - and the RGB image Pillow decodes from each.  Packed like
jpeg_streams.npz: the files and the images as one byte vector each, plus the file ends and the names; tests/jpegd_cases.py
foreign_files() takes them apart again.
    python tests/golden/make_jpegd_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402
import jpegd_cases  # noqa: E402


def pillow(case):
    """-> (file bytes, decoded uint8 (h, w, 3))."""
    buf = io.BytesIO()
    args = dict(format='JPEG', subsampling=jpeg_cases.SUBSAMPLINGS.index(case.subsampling), optimize=case.optimize)
    if case.qtables:
        args['qtables'] = [list(t) for t in jpegd_cases.QTABLES[case.qtables]]
    else:
        args['quality'] = case.quality
    Image.fromarray(jpegd_cases.foreign_image(case)).save(buf, **args)
    return buf.getvalue(), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))


def main():
    done = [pillow(case) for case in jpegd_cases.FOREIGN]
    np.savez_compressed(jpegd_cases.GOLDEN, names=np.array([c.name for c in jpegd_cases.FOREIGN]),
                        rgb=np.concatenate([d[1].reshape(-1) for d in done]), files=np.frombuffer(b''.join(d[0] for d in done), np.uint8),
                        file_ends=np.cumsum([len(d[0]) for d in done]).astype(np.int64))
    print(jpegd_cases.GOLDEN, os.path.getsize(jpegd_cases.GOLDEN), 'bytes;', len(done), 'files')


if __name__ == '__main__':
    main()
