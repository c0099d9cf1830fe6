"""Writes tests/golden/jpeg_scaled.npz: for every case of tests/jpegscale_cases.py the files Pillow (libjpeg-turbo) writes for its image -
baseline, and for some progressive and with restart intervals - and, for every scale in 1, 2, 4, 8 that Pillow can be asked for, the
image it decodes from the baseline file after Image.draft(): the CRC32 of every one, and the pixels themselves of all but the large
case.  The script asserts that Pillow chose the scale it was meant to (im.decoderconfig[0]), that every variant of a case decodes to the
same pixels at every scale, that the restated file is Pillow's (so the restatement's coefficients are the file's), and holds the
restatement (tests/jpegscale_ref.py) to every image while writing.  It also records Pillow's choice of scale for further requests.
    python tests/golden/make_jpegscale_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpegscale_cases as cases  # noqa: E402


def write(case, variant):
    img = np.asarray(cases.build(case))
    how = {} if case.sampling == 'L' else dict(subsampling=case.sampling)
    buf = io.BytesIO()
    Image.fromarray(img, 'L' if case.sampling == 'L' else 'RGB').save(
        buf, format='JPEG', quality=case.quality, progressive=variant == 'prog',
        restart_marker_blocks=cases.RESTART_BLOCKS if variant == 'rst' else 0, **how)
    return buf.getvalue()


def draft(data, size):
    """The file opened and asked for `size` (width, height; None = no draft): (the scale Pillow chose, the decoded uint8 image with
    a last axis)."""
    im = Image.open(io.BytesIO(data))
    mode = im.mode
    scale = 1
    if size is not None and im.draft(mode, size) is not None:
        scale = im.decoderconfig[0]
    px = np.asarray(im)
    assert im.mode == mode
    return scale, px.reshape(px.shape[0], px.shape[1], -1)


def main():
    files, crcs, pixels, checked = [], np.zeros((len(cases.CASES), len(cases.SCALES)), np.uint32), [], 0
    for i, case in enumerate(cases.CASES):
        made = {v: write(case, v) for v in case.variants}
        assert made['plain'] == cases.restated_file(case), case.name
        files += [made[v] for v in case.variants]
        for j, s in enumerate(cases.SCALES):
            if not cases.askable(case, s):
                continue
            got = None
            for v in case.variants:
                scale, px = draft(made[v], cases.request(case, s))
                assert scale == s, (case.name, v, s, scale)
                assert px.shape[:2] == cases.sref.scaled_size(case.h, case.w, s), (case.name, s, px.shape)
                assert got is None or np.array_equal(got, px), (case.name, v, s)
                got = px
            assert np.array_equal(got, cases.expected(case, s)), ('the restatement differs from Pillow', case.name, s)
            checked += 1
            crcs[i, j] = cases.crc(got)
            if cases.pixels_held(case, s):
                pixels.append(got.reshape(-1))
    by_size = {(c.h, c.w): c for c in cases.CASES if c.sampling == '4:2:0'}
    rows = []
    for case in cases.CASES:
        rows += [(case.h, case.w) + cases.request(case, s) + (s,) for s in cases.SCALES if cases.askable(case, s)]
    for h, w, rw, rh in cases.DRAFT_REQUESTS:
        rows.append((h, w, rw, rh, draft(write(by_size[(h, w)], 'plain'), (rw, rh))[0]))
    np.savez_compressed(cases.GOLDEN, names=np.array(cases.IDS), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64), crcs=crcs, pixels=np.concatenate(pixels),
                        draft=np.array(sorted(set(rows)), np.int32))
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes;', len(cases.CASES), 'cases,', len(files), 'files,', checked,
          'images equal to the restatement')
    assert os.path.getsize(cases.GOLDEN) < 184009          # golden/jpeg_grey_streams.npz


if __name__ == '__main__':
    main()
