"""Writes tests/golden/jpeg_lossless.npz: the source files of tests/jpegxform_cases.py - Pillow's (libjpeg-turbo's) 4:4:4, 4:2:2, 4:2:0
and 'L' files, baseline, optimised, progressive and with restart intervals, and the test writer's files of the wide samplings - and, for
every (file, operation, edge, crop) case, the output file the restatement (tests/jpegxform_ref.py) makes, the pixels Pillow decodes
from that output file, and the Image.size and Image.layer (component id, h, v, table) Pillow reports for it.  Pillow is the judge of
what an output file shows; the script only asserts what must hold: that Pillow opens every file at the expected size and factors, and
that a vertical flip of a file without vertical chroma interpolation decodes to the flipped source decode bit for bit.
    python tests/golden/make_jpegxform_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpegxform_cases as cases  # noqa: E402
import jpegxform_ref as xr  # noqa: E402


def main():
    sources = {s.name: cases.make_source(s) for s in cases.SOURCES}
    files, sizes, layers, crcs, pixels, refused = [], [], [], [], [], 0
    for case in cases.FILE_CASES:
        s = case.source
        want = cases.expected_size(case)
        if want is None:
            files.append(b'')
            sizes.append((0, 0, 0))
            layers.append(np.zeros((3, 4), np.int32))
            crcs.append(0)
            refused += 1
            continue
        data = xr.transcode(sources[s.name], case.op, case.crop, case.edge)
        im = Image.open(io.BytesIO(data))
        px = np.asarray(im)
        nc = 1 if s.sampling == 'grey' else 3
        assert im.size == (want[1], want[0]) and im.mode == ('L' if nc == 1 else 'RGB'), (case.name, im.size, im.mode)
        assert im.layer[0][1:3] == ((1, 1) if nc == 1 else want[2:]), (case.name, im.layer)
        if case.op == 'vflip' and case.crop is None and want[3] in (0, 1) and want[0] == s.h:
            assert np.array_equal(px, np.asarray(Image.open(io.BytesIO(sources[s.name])))[::-1]), case.name
        layer = np.zeros((3, 4), np.int32)
        layer[:nc] = np.array(im.layer, np.int32)
        files.append(data)
        sizes.append((im.size[0], im.size[1], nc))
        layers.append(layer)
        crcs.append(cases.crc(px))
        if px.shape[0] * px.shape[1] <= cases.PIXELS_UP_TO:
            pixels.append(px.reshape(-1))
    ordered = [sources[s.name] for s in cases.SOURCES]
    np.savez_compressed(cases.GOLDEN, sources=np.array([s.name for s in cases.SOURCES]), cases=np.array(cases.FILE_IDS),
                        source_files=np.frombuffer(b''.join(ordered), np.uint8),
                        source_ends=np.cumsum([len(f) for f in ordered]).astype(np.int64),
                        files=np.frombuffer(b''.join(files), np.uint8), file_ends=np.cumsum([len(f) for f in files]).astype(np.int64),
                        sizes=np.array(sizes, np.int32), layers=np.stack(layers), crcs=np.array(crcs, np.uint32),
                        pixels=np.concatenate(pixels))
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes;', len(cases.SOURCES), 'source files,', len(files) - refused, 'output files,',
          refused, 'cases refused')
    assert os.path.getsize(cases.GOLDEN) < 200000


if __name__ == '__main__':
    main()
