"""Times ops.jpeg_lossless against a device-to-device copy of the same tensor - the copy moves exactly the bytes
the kernel must -, and the share of the launch in a whole transcode_batch(optimize=True, lossless=) call.  HIP events after warm-up.
    python tools/jpeg_lossless_time.py [--n 16] [--side 2048] [--reps 50] [--files 16] [--file-side 512]
Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module('neural-imaging_amd')
from neural_imaging_amd import ops  # noqa: E402
from neural_imaging_amd.compression import jpeg_helpers as jh  # noqa: E402


def timed(fn, reps):
    """Median and minimum milliseconds of fn() over `reps` event-timed runs, after three warm-up runs."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--side', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--files', type=int, default=16)
    ap.add_argument('--file-side', type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('needs a GPU')
    dev = torch.device('cuda', 0)
    hs, vs, side = 2, 2, args.side
    nb = ops.jpeg_geometry(side, side, hs, vs)[0]
    coef = torch.randint(-1024, 1024, (args.n, nb, 64), dtype=torch.int16, device=dev)
    out = torch.empty_like(coef)
    result = {'n': args.n, 'side': side, 'sampling': '4:2:0', 'tensor_bytes': coef.numel() * 2}
    result['copy_ms'], result['copy_min_ms'] = timed(lambda: out.copy_(coef), args.reps)
    for op in ('hflip', 'transpose', 'rot90'):
        med, low = timed(lambda: ops.jpeg_lossless(coef, side, side, hs, vs, op, out=out), args.reps)
        result[op + '_ms'], result[op + '_min_ms'], result[op + '_over_copy'] = med, low, med / result['copy_ms']
        result[op + '_GBps'] = 2 * result['tensor_bytes'] / med / 1e6
    result['copy_GBps'] = 2 * result['tensor_bytes'] / result['copy_ms'] / 1e6

    # the share of the launch in a whole call: files of one geometry, natural-like content
    fs = args.file_side
    y, x = np.mgrid[:fs, :fs]
    rng = np.random.default_rng(1)
    batch = np.stack([np.clip(np.stack([128 + 100 * np.sin(x / (7.0 + k)) * np.cos(y / 5.0), 255.0 * x / fs, 255.0 * (x + y) / (2 * fs)], -1)
                              + rng.normal(0, 8, (fs, fs, 3)), 0, 255).astype(np.uint8) for k in range(args.files)])
    files = jh.encode_batch(batch, 85, '4:2:0')
    for _ in range(2):
        jh.transcode_batch(files, lossless='rot90')
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t = time.perf_counter()
        jh.transcode_batch(files, lossless='rot90')
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t))
    small = torch.randint(-64, 64, (args.files, ops.jpeg_geometry(fs, fs, hs, vs)[0], 64), dtype=torch.int16, device=dev)
    launch, _ = timed(lambda: ops.jpeg_lossless(small, fs, fs, hs, vs, 'rot90'), args.reps)
    result.update(files=args.files, file_side=fs, transcode_rot90_ms=float(np.median(walls)), lossless_in_call_ms=launch,
                  lossless_share=launch / float(np.median(walls)))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
