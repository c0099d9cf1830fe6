"""Writes tests/golden/jpeg_rst_streams.npz: for every case of tests/jpegrst_cases.py and each of its variants the whole file Pillow
(libjpeg) writes for each image - Image.save(format='JPEG', restart_marker_blocks=Ri, ...) with quality= or qtables=, optimize= - and
the image Pillow decodes from the plain file.  It pins the writer with restart intervals to libjpeg, and gives the reader foreign
files with restart markers, on machines without Pillow.  The inputs are rebuilt by jpegrst_cases.build, so no source pixels are
stored; tests/jpegrst_cases.py golden() takes the file apart again.
    python tests/golden/make_jpegrst_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402
import jpegrst_cases  # noqa: E402


def pillow(img, case, variant):
    """uint8 (h, w, 3) -> (the bytes of the file of `variant`, the uint8 image decoded from it)."""
    ri, optimize, qt = jpegrst_cases.variant_settings(case, variant)
    how = dict(quality=case.quality) if qt is None else dict(qtables=[[int(v) for v in t] for t in qt])
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, format='JPEG', subsampling=jpeg_cases.SUBSAMPLINGS.index(case.subsampling),
                                          optimize=optimize, restart_marker_blocks=ri, **how)
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def main():
    files, rgb = [], []
    for case in jpegrst_cases.CASES:
        for variant in case.variants:
            done = [pillow(img, case, variant) for img in jpegrst_cases.build(case)]
            files += [d[0] for d in done]
            if variant == 'plain':
                rgb += [d[1].reshape(-1) for d in done]
    np.savez_compressed(jpegrst_cases.GOLDEN, names=np.array(jpegrst_cases.IDS), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64), rgb=np.concatenate(rgb))
    print(jpegrst_cases.GOLDEN, os.path.getsize(jpegrst_cases.GOLDEN), 'bytes;', len(jpegrst_cases.CASES), 'cases,', len(files), 'files')
    assert os.path.getsize(jpegrst_cases.GOLDEN) < 512 * 1024


if __name__ == '__main__':
    main()
