"""Writes tests/golden/jpegdprog_streams.npz for the progressive decoder's tests: the files of scan scripts A and B (jpegdprog_ref)
that tests/jpegdprog_ref.encode writes for the cases of jpegdprog_cases.SCRIPT_CASES, and - for them and for the 72 Pillow files of
jpegprog_streams.npz - the CRC32 of the RGB image Pillow (libjpeg) decodes from each.  It pins the decoder's pixels to libjpeg on
machines without Pillow, and shows that libjpeg reads the files of the two scripts: each must decode to exactly the pixels of
Pillow's own progressive file of the same image.
    python tests/golden/make_jpegdprog_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpegdprog_cases as cases  # noqa: E402
import jpegprog_cases  # noqa: E402


def decoded(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def main():
    names, files, crc_names, crcs = [], [], [], []
    for name, group in jpegprog_cases.golden().items():
        for i, data in enumerate(group):
            crc_names.append('{}|{}|std'.format(name, i))
            crcs.append(cases.crc(decoded(data)))
    for script in ('A', 'B'):
        for name in cases.SCRIPT_CASES:
            data = cases.script_file(name, script)
            rgb = decoded(data)
            assert np.array_equal(rgb, decoded(jpegprog_cases.golden()[name][0])), (name, script)
            names.append('{}|{}'.format(name, script))
            files.append(data)
            crc_names.append('{}|0|{}'.format(name, script))
            crcs.append(cases.crc(rgb))
    np.savez_compressed(cases.GOLDEN, names=np.array(names), files=np.frombuffer(b''.join(files), np.uint8),
                        file_ends=np.cumsum([len(f) for f in files]).astype(np.int64), crc_names=np.array(crc_names),
                        crcs=np.array(crcs, np.uint32))
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes;', len(files), 'files,', len(crcs), 'checksums')
    assert os.path.getsize(cases.GOLDEN) < 100000


if __name__ == '__main__':
    main()
