"""Writes tests/golden/jpeg_sampling.npz: for every case of tests/jpegsamp_cases.py the files the test writer (tests/jpegsamp_ref.py)
produces for its variants and, for every scale in 1, 2, 4, 8 that Pillow (libjpeg-turbo) can be asked for, the image Pillow decodes from
them after Image.draft(): the CRC32 of every one, and the pixels themselves of the small ones.  The script asserts that Pillow chose
the scale it was meant to (im.decoderconfig[0]), that every variant of a case decodes to the same pixels at every scale, and holds the
restatement to every image while writing: Pillow is the judge of the restatement, never the other way round.
    python tests/golden/make_jpegsamp_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpegsamp_cases as cases  # noqa: E402


def draft(data, size):
    """The file opened and asked for `size` (width, height; None = no draft): (the scale Pillow chose, the decoded uint8 image)."""
    im = Image.open(io.BytesIO(data))
    scale = 1
    if size is not None and im.draft('RGB', size) is not None:
        scale = im.decoderconfig[0]
    px = np.asarray(im)
    assert im.mode == 'RGB'
    return scale, px


def main():
    files, crcs, pixels, checked = [], np.zeros((len(cases.CASES), len(cases.SCALES)), np.uint32), [], 0
    for i, case in enumerate(cases.CASES):
        made = {v: cases.written(case, v) for v in case.variants}
        files += [made[v] for v in case.variants]
        for j, s in enumerate(cases.SCALES):
            if not cases.askable(case, s):
                continue
            got = None
            for v in case.variants:
                scale, px = draft(made[v], None if s == 1 else cases.request(case, s))
                assert scale == s, (case.name, v, s, scale)
                assert px.shape == (-(-case.h // s), -(-case.w // s), 3), (case.name, s, px.shape)
                assert got is None or np.array_equal(got, px), (case.name, v, s)
                got = px
            assert np.array_equal(got, cases.expected(case, s)), ('the restatement differs from Pillow', case.name, s)
            checked += 1
            crcs[i, j] = cases.crc(got)
            if cases.pixels_held(case, s):
                pixels.append(got.reshape(-1))
    np.savez_compressed(cases.GOLDEN, names=np.array(cases.IDS), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64), crcs=crcs, pixels=np.concatenate(pixels))
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes;', len(cases.CASES), 'cases,', len(files), 'files,', checked,
          'images equal to the restatement')
    assert os.path.getsize(cases.GOLDEN) < 184009          # golden/jpeg_grey_streams.npz, the largest JPEG fixture


if __name__ == '__main__':
    main()
