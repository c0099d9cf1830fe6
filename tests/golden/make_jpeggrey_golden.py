"""Writes tests/golden/jpeg_grey_streams.npz: for every case of tests/jpeggrey_cases.py and each of its variants the whole file Pillow
(libjpeg) writes for each mode 'L' image - Image.save(format='JPEG', quality= or qtables=, optimize=, restart_marker_blocks=,
progressive=, subsampling=) - and the image Pillow decodes from the case's first variant.  It pins the grey-scale writer to libjpeg and
gives the reader foreign files - baseline, progressive and with the factors 2x2 declared - on machines without Pillow.  The inputs are
rebuilt by jpeggrey_cases.build, so no source pixels are stored; jpeggrey_cases.golden() takes the file apart again.  While writing,
the restatement (tests/jpeggrey_ref.py) is held to every file and to the decoded pixels.
    python tests/golden/make_jpeggrey_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeggrey_cases as cases  # noqa: E402


def pillow(img, case, variant):
    """uint8 (h, w) -> (the bytes of the file of `variant`, the uint8 (h, w) image decoded from it)."""
    how = dict(quality=case.quality) if not case.qt else dict(qtables=[[int(v) for v in cases.QTABLES[case.qt]]])
    if variant == 's22':
        how['subsampling'] = 2
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img), 'L').save(buf, format='JPEG', optimize=variant == 'opt', progressive=variant == 'prog',
                                               restart_marker_blocks=case.ri, **how)
    data = buf.getvalue()
    back = Image.open(io.BytesIO(data))
    assert back.mode == 'L'
    return data, np.asarray(back)


def main():
    files, pixels = [], []
    for case in cases.CASES:
        for variant in case.variants:
            done = [pillow(img, case, variant) for img in cases.build(case)]
            assert [d[0] for d in done] == cases.restated(case, variant)[0], (case.name, variant)
            assert all(np.array_equal(d[1], want) for d, want in zip(done, cases.decoded(case))), (case.name, variant)
            files += [d[0] for d in done]
            if variant == case.variants[0]:
                pixels += [d[1].reshape(-1) for d in done]
    np.savez_compressed(cases.GOLDEN, names=np.array(cases.IDS), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64), pixels=np.concatenate(pixels))
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes;', len(cases.CASES), 'cases,', len(files), 'files')
    assert os.path.getsize(cases.GOLDEN) < 214364          # the largest golden file before this one


if __name__ == '__main__':
    main()
