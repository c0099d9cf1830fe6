"""Writes tests/golden/jpeg_streams.npz: for every golden case of tests/jpeg_cases.py the uint8 input batch, the whole file Pillow
(libjpeg) writes for each image with default settings and the RGB image Pillow decodes from it.  It pins the baseline JPEG codec
to libjpeg on machines without Pillow.  Everything is packed into three byte vectors in case order (x, rgb, files) - one zip
member each, so that the 623 header bytes every file repeats compress away - plus the file ends and the case names;
tests/jpeg_cases.py golden() takes them apart again.
    python tests/golden/make_jpeg_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402


def pillow(img, quality, subsampling):
    """uint8 (h, w, 3) -> (file bytes, decoded uint8 (h, w, 3))."""
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling=jpeg_cases.SUBSAMPLINGS.index(subsampling))
    return buf.getvalue(), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))


def main():
    names, xs, rgbs, files = [], [], [], []
    for case in jpeg_cases.GOLDEN_CASES:
        x = jpeg_cases.build(case)
        done = [pillow(img, case.quality, case.subsampling) for img in x]
        names.append(case.name)
        xs.append(x.reshape(-1))
        rgbs.append(np.stack([d[1] for d in done]).reshape(-1))
        files += [d[0] for d in done]
    np.savez_compressed(jpeg_cases.GOLDEN, names=np.array(names), x=np.concatenate(xs), rgb=np.concatenate(rgbs),
                        files=np.frombuffer(b''.join(files), np.uint8), file_ends=np.cumsum([len(f) for f in files]).astype(np.int64))
    print(jpeg_cases.GOLDEN, os.path.getsize(jpeg_cases.GOLDEN), 'bytes;', len(names), 'cases,', len(files), 'files')


if __name__ == '__main__':
    main()
