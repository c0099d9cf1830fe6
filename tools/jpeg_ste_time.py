"""
Times the real codec as a training forward (nimg_jpeg_ste_fwd) next to what it replaces and what it is shaped
like, in one process, with device events around each call, after a warm-up, the legs alternating within every repetition:
  ste_mask / ste_nomask   ops.jpeg_ste_fwd with and without the clip mask
  pair                    ops.jpeg_transform_tables + ops.jpeg_reconstruct_tables on the same input and tables: the same image, no mask
  djpeg_mask              ops.djpeg_fwd / ops.djpeg_sub_fwd (the float model, 'soft') with its mask
at 4:4:4, 4:2:2 and 4:2:0 on natural images.  Prints one JSON line per sub-sampling: median [min .. max] milliseconds per leg, the
algorithmic bytes per pixel of the fused call (x 12 + y 12 + mask 1; sub-sampled: x a second time, 12, and the reduced planes written
and read back, 2 * 2 / (hs vs)) and the GB/s that gives at the median.  The image of the fused call is checked against the pair's.

    python tools/jpeg_ste_time.py [--batch 320] [--size 256] [--quality 75] [--reps 15]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
importlib.import_module('neural-imaging_amd')
from neural_imaging_amd import ops  # noqa: E402
from neural_imaging_amd.compression import jpeg_helpers  # noqa: E402
from util import natural_images  # noqa: E402
from src_stamp import csrc_sha16  # noqa: E402

SUBSAMPLINGS = ('4:4:4', '4:2:2', '4:2:0')


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(x, quality, subsampling, reps, warmup=3):
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x.shape
    dev = x.device
    t3 = np.stack([jpeg_helpers.libjpeg_qtable(quality, c).ravel() for c in (0, 1, 1)])
    one = torch.from_numpy(t3.astype(np.int16).reshape(1, 3, 64)).to(dev)
    per_item = one.repeat(n, 1, 1).contiguous()
    qf = torch.from_numpy(t3.astype(np.float32).reshape(3, 8, 8)).to(dev)
    y, y2 = torch.empty_like(x), torch.empty_like(x)
    ws_ste = torch.empty(max(ops.jpeg_ste_workspace_bytes(n, h, w, hs, vs), 1), dtype=torch.uint8, device=dev)
    ws_pair = torch.empty(ops.jpeg_workspace_bytes(n, h, w, hs, vs), dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def pair():
        coef, _ = ops.jpeg_transform_tables(x, per_item, hs, vs, workspace=ws_pair, err=err)
        ops.jpeg_reconstruct_tables(coef, h, w, per_item, hs, vs, workspace=ws_pair, out=y2)
    legs = {
        'ste_mask': lambda: ops.jpeg_ste_fwd(x, one, hs, vs, want_mask=True, out=y, workspace=ws_ste, err=err),
        'ste_nomask': lambda: ops.jpeg_ste_fwd(x, one, hs, vs, want_mask=False, out=y, workspace=ws_ste, err=err),
        'pair': pair,
        'djpeg_mask': (lambda: ops.djpeg_fwd(x, qf, 'soft', want_mask=True, out=y2)) if (hs, vs) == (1, 1) else
                      (lambda: ops.djpeg_sub_fwd(x, qf, 'soft', hs, vs, want_mask=True, out=y2)),
    }
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    legs['ste_mask']()
    pair()
    assert torch.equal(y, y2), 'the fused call and the pair disagree'
    times = {k: [] for k in legs}
    for _ in range(reps):                                # alternating: every leg once per repetition
        for k, fn in legs.items():
            times[k].append(once(fn))
    extra = 0.0 if hs == 1 else 12.0 + 4.0 / (hs * vs)        # sub-sampled: both passes read x; the reduced planes go out and come back
    bpp = {'ste_mask': 25.0 + extra, 'ste_nomask': 24.0 + extra}
    ms = {k: {'median': round(float(np.median(v)), 4), 'min': round(float(np.min(v)), 4), 'max': round(float(np.max(v)), 4)}
          for k, v in times.items()}
    return {'mode': 'jpeg_ste', 'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality, 'reps': reps, 'ms': ms,
            'bytes_per_pixel': bpp, 'gb_per_s': {k: round(bpp[k] * n * h * w / ms[k]['median'] / 1e6, 1) for k in bpp}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=320)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--quality', type=int, default=75)
    ap.add_argument('--reps', type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_ste_time.py needs a GPU')
    dev = torch.device('cuda', 0)
    base = natural_images(min(args.batch, 32), args.size, args.size, seed=1)          # 32 distinct images, repeated to the batch
    x = torch.from_numpy(np.concatenate([base] * -(-args.batch // len(base)))[:args.batch]).to(dev)
    for subsampling in SUBSAMPLINGS:
        print(json.dumps(dict(measure(x, args.quality, subsampling, args.reps), csrc_sha16=csrc_sha16())), flush=True)


if __name__ == '__main__':
    main()
