"""Writes tests/golden/jpegprog_streams.npz: for every case of tests/jpegprog_cases.py the whole file Pillow (libjpeg) writes for each
image with Image.save(format='JPEG', progressive=True, ...) - quality= or qtables=, restart_marker_blocks=.  It pins the progressive
writer to libjpeg on machines without Pillow.  The inputs are rebuilt by jpegprog_cases.build, so no pixels are stored;
jpegprog_cases.golden() takes the file apart again.  While it writes, it checks the plain Python restatement on the slow cases (the
flat 512x4096 image: a run of exactly 0x7fff blocks, then a run of 1), that progressive=True with optimize=True gives the same
bytes, and that Pillow decodes every file to the pixels of its baseline file.
    python tests/golden/make_jpegprog_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402
import jpegprog_cases  # noqa: E402


def pillow(img, case, progressive=True, optimize=False):
    """uint8 (h, w, 3) -> (the bytes of the file, the uint8 image decoded from it)."""
    qt = jpegprog_cases.qtables(case)
    how = dict(quality=case.quality) if qt is None else dict(qtables=[[int(v) for v in t] for t in qt])
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, format='JPEG', subsampling=jpeg_cases.SUBSAMPLINGS.index(case.subsampling),
                                          progressive=progressive, optimize=optimize, restart_marker_blocks=case.ri, **how)
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def main():
    files = []
    for case in jpegprog_cases.CASES:
        for i, img in enumerate(jpegprog_cases.build(case)):
            data, decoded = pillow(img, case)
            assert data == pillow(img, case, optimize=True)[0], case.name
            assert np.array_equal(decoded, pillow(img, case, progressive=False)[1]), case.name
            if case.slow:
                assert jpegprog_cases.reference(case).files[i] == data, case.name
                print(case.name, jpegprog_cases.reference(case).stats)
            files.append(data)
    np.savez_compressed(jpegprog_cases.GOLDEN, names=np.array(jpegprog_cases.IDS), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64))
    print(jpegprog_cases.GOLDEN, os.path.getsize(jpegprog_cases.GOLDEN), 'bytes;', len(jpegprog_cases.CASES), 'cases,', len(files), 'files')
    assert os.path.getsize(jpegprog_cases.GOLDEN) <= 214364          # jpeg_rst_streams.npz, the largest golden file before it


if __name__ == '__main__':
    main()
