"""
Times the baseline JPEG codec (neural_imaging_amd.compression.jpeg_helpers over nimg_jpeg_*) for one configuration with device
events, after a warm-up:
  transform    RGB -> quantised coefficients (one kernel; float input: plus the scan for a value above 1)
  encode       coefficients -> entropy-coded segments and their lengths (seven kernels, one nimg_jpeg_encode call)
  copy_d2h     the lengths, then the segments, device to host
  reconstruct  coefficients -> decoded float32 images (two kernels)
  compress_batch_total   jpeg_helpers.compress_batch on the host batch: upload, the three stages, both downloads
at 4:4:4 and at 4:2:0, on natural images.  Prints one JSON line per sub-sampling.  --pillow adds the host's time for the same
images through Pillow (libjpeg), one after the other, where Pillow is installed; it needs no GPU.
--decode times the way back on the files encode_batch writes for the same images: nimg_jpeg_decode as a whole
and per kernel (prepare, speculate, sync, write, dc - from the profiler's kernel records), the synchronisation rounds,
nimg_jpeg_reconstruct_tables and decode_batch from bytes to bytes, at subseq_bits 256, 512, 1024, 2048 and at one subsequence per
image - the sequential decode the parallel one is measured against.  One JSON line per sub-sampling and setting.
--optimize times writing with optimised Huffman tables: nimg_jpeg_histogram, nimg_jpeg_optimal_tables and
nimg_jpeg_encode_tables next to nimg_jpeg_encode on the same coefficients, encode_batch with and without optimize from host batch
to files, and the segment and whole-file bytes either way.  One JSON line per sub-sampling.
--progressive times writing progressive files: nimg_jpeg_progressive_histogram, nimg_jpeg_optimal_tables on
the 10 n histograms and nimg_jpeg_encode_progressive next to nimg_jpeg_encode_tables on the same coefficients, encode_batch with
progressive=True from host batch to files, and the bytes of the baseline, the optimised and the progressive files.  One JSON line
per sub-sampling.
--qtables times the table form with libjpeg's tables of --quality, so that its numbers stand next to the
default mode's: nimg_jpeg_transform_tables (the divisors read from device memory), nimg_jpeg_encode on its coefficients,
nimg_jpeg_reconstruct_tables and compress_batch(qtables=); the coefficients are checked against the quality form's.  One JSON line
per sub-sampling.

--restart N / --restart-rows R give the files a restart interval of N MCUs / of R MCU rows at either
sub-sampling: the default mode then times nimg_jpeg_encode_restart and compress_batch(restart_interval=), and --decode times
nimg_jpeg_decode_restart and decode_batch(allow_restart=True) on those files.  Every line names its interval.
--decode-progressive times reading progressive files on the files encode_batch(progressive=True) writes for
the same images: nimg_jpeg_decode_progressive as a whole and per kernel kind (prepare, first scans, DC refine, AC refine - from the
profiler's kernel records), the synchronisation rounds of the first scans, and decode_batch(allow_progressive=True) from bytes to
bytes next to decode_batch on the baseline twins of the same coefficients (encode_batch(optimize=True)) in the same process, at
subseq_bits 256, 512, 1024, 2048 and at one subsequence per scan and interval.  One JSON line per sub-sampling and setting.

    python tools/jpeg_time.py --batch 64 --size 256 --quality 75 [--reps 20]
                              [--pillow | --decode | --decode-progressive | --optimize | --progressive | --qtables]
                              [--restart N | --restart-rows R]
For the split of the calls into their kernels: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/jpeg_time.py ...
"""
import argparse
import importlib
import io
import json
import os
import sys
import time

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

SUBSAMPLINGS = ('4:4:4', '4:2:0')


def timed(fn, reps):
    """median milliseconds of fn() between device events, and its last result"""
    out, times = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), out


def interval_of(args, h, w, subsampling):
    """the restart interval in MCUs the arguments ask for at this sub-sampling"""
    hs, _ = ops.jpeg_subsampling(subsampling)
    return args.restart_rows * -(-w // (8 * hs)) if args.restart_rows else args.restart


def measure(x_host, quality, subsampling, reps, dev, ri=0):
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x_host.shape
    x = torch.from_numpy(x_host).to(dev)
    ws = torch.empty(ops.jpeg_workspace_bytes(n, h, w, hs, vs, ri), dtype=torch.uint8, device=dev)
    out = torch.empty(n * (192 * ops.jpeg_geometry(h, w, hs, vs)[1] + 1024), dtype=torch.uint8, device=dev)
    ms = {}
    ms['transform'], coef = timed(lambda: ops.jpeg_transform(x, quality, hs, vs, workspace=ws), reps)
    ms['encode'], (data, lengths) = timed(lambda: ops.jpeg_encode(coef, h, w, hs, vs, out=out, workspace=ws, restart_interval=ri), reps)

    def copy_out():
        ln = lengths.cpu().numpy().astype(np.int64)
        return data[:int(ln.sum())].cpu().numpy(), ln
    ms['copy_d2h'], (blob, ln) = timed(copy_out, reps)
    ms['reconstruct'], y = timed(lambda: ops.jpeg_reconstruct(coef, h, w, quality, hs, vs, workspace=ws), reps)
    ms['compress_batch_total'], (yb, sizes) = timed(
        lambda: jpeg_helpers.compress_batch(x_host, quality, subsampling=subsampling, restart_interval=ri), reps)
    assert np.array_equal(yb, y.cpu().numpy()) and sizes == (ln + jpeg_helpers._header_bytes(None, ri)[0] + 2).tolist()
    return {'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality, 'restart_interval': ri, 'bytes': int(ln.sum()),
            'bpp': 8.0 * float(np.mean(sizes)) / h / w, 'ms': {k: round(v, 4) for k, v in ms.items()},
            'images_per_s': {k: n / v * 1e3 for k, v in ms.items()}}


# stage -> what its kernel's name holds in the profiler's records, demangled or mangled
DECODE_STAGES = (('prepare', ('jpegd_prepare_kernel',)), ('speculate', ('jpegd_decode_kernel<false', 'jpegd_decode_kernelILb0E')),
                 ('sync', ('jpegd_sync_kernel',)), ('write', ('jpegd_decode_kernel<true', 'jpegd_decode_kernelILb1E')),
                 ('dc', ('jpegd_dc_kernel',)))


def kernel_ms(fn, reps, stages=None):
    """mean milliseconds per call of every decoder kernel, from the profiler's device records; None where it records none"""
    stages = DECODE_STAGES if stages is None else stages
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        events = [(e.name, e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total) for e in prof.events()]
    except Exception:
        return None
    out = {}
    for stage, keys in stages:
        times = [t for name, t in events if any(k in name for k in keys)]
        if not times:                                                # a stage without a record: no partial table
            return None
        out[stage] = round(sum(times) / reps / 1e3, 4)
    return out


def measure_decode(x_host, quality, subsampling, reps, dev, ri=0):
    """one dict per subseq_bits setting"""
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x_host.shape
    files = jpeg_helpers.encode_batch(x_host, quality, subsampling, restart_interval=ri)
    heads = [jpeg_helpers.parse_header(f, allow_restart=True) for f in files]
    segments = [f[hd.ecd_offset:hd.ecd_end] for f, hd in zip(files, heads)]
    ecd = torch.from_numpy(np.frombuffer(b''.join(segments), np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64)).to(dev)
    huff = np.zeros((n, 6, 272), np.uint8)
    for t, (counts, symbols) in enumerate(heads[0].huffman):
        huff[:, t, :16], huff[:, t, 16:16 + len(symbols)] = np.frombuffer(counts, np.uint8), np.frombuffer(symbols, np.uint8)
    huff = torch.from_numpy(huff).to(dev)
    qt = torch.from_numpy(np.stack([hd.qtables for hd in heads]).view(np.int16)).to(dev)
    want = ops.jpeg_transform(torch.from_numpy(x_host).to(dev), quality, hs, vs)
    whole = -(-8 * max(len(s) for s in segments) // 32) * 32
    rows = []
    for subseq_bits in (256, 512, 1024, 2048, whole):
        size = int(ops._lib.load().nimg_jpeg_decode_restart_workspace_bytes(n, h, w, hs, vs, ri, ecd.numel(), subseq_bits))
        ws = torch.empty(size, dtype=torch.uint8, device=dev)

        def decode():
            return ops.jpeg_decode(ecd, off, huff, h, w, hs, vs, subseq_bits=subseq_bits, workspace=ws, restart_interval=ri)
        ms = {}
        ms['decode'], (coef, status, rounds) = timed(decode, reps)
        assert int(status.abs().sum()) == 0 and torch.equal(coef, want)
        ms['reconstruct_tables'], y = timed(lambda: ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs, out_u8=True), reps)
        ms['decode_batch_total'], yb = timed(lambda: jpeg_helpers.decode_batch(files, subseq_bits=subseq_bits, allow_restart=True),
                                             max(3, reps // 4))
        assert np.array_equal(yb, y.cpu().numpy())
        r = rounds.cpu().numpy()
        rows.append({'mode': 'decode', 'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality,
                     'restart_interval': ri, 'subseq_bits': subseq_bits, 'sequential': subseq_bits == whole, 'segment_bytes': int(ecd.numel()),
                     'subsequences_per_image': round(8.0 * ecd.numel() / n / subseq_bits, 1), 'workspace_bytes': size,
                     'rounds': {'min': int(r.min()), 'median': float(np.median(r)), 'max': int(r.max())},
                     'ms': {k: round(v, 4) for k, v in ms.items()}, 'kernel_ms': kernel_ms(decode, reps),
                     'images_per_s': {k: n / v * 1e3 for k, v in ms.items()}})
    return rows


PROGRESSIVE_STAGES = (('prepare', ('jpegd_prog_prepare_kernel',)), ('first', ('jpegd_prog_first_kernel',)),
                      ('dc_refine', ('jpegd_prog_dc_refine_kernel',)), ('ac_refine', ('jpegd_prog_ac_refine_kernel',)))


def measure_decode_progressive(x_host, quality, subsampling, reps, dev):
    """one dict per subseq_bits setting"""
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x_host.shape
    files = jpeg_helpers.encode_batch(x_host, quality, subsampling, progressive=True)
    twins = jpeg_helpers.encode_batch(x_host, quality, subsampling, optimize=True)
    heads = [jpeg_helpers.parse_header(f, allow_progressive=True) for f in files]
    script = [s[:5] for s in heads[0].scans]
    assert all([s[:5] for s in hd.scans] == script for hd in heads)
    rows6 = np.array([[sum(1 << c for c in cs), ss, se, ah, al, lv]
                      for (cs, ss, se, ah, al), lv in zip(script, jpeg_helpers.jpeg_script_check(script))], np.int32)
    segments = [f[s.ecd_offset:s.ecd_end] for f, hd in zip(files, heads) for s in hd.scans]
    ecd = torch.from_numpy(np.frombuffer(b''.join(segments), np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64)).to(dev)
    huff = np.zeros((n, len(script), 3, 272), np.uint8)
    for i, hd in enumerate(heads):
        for k, sc in enumerate(hd.scans):
            for c, (counts, symbols) in enumerate(sc.huffman):
                huff[i, k, c, :16], huff[i, k, c, 16:16 + len(symbols)] = np.frombuffer(counts, np.uint8), np.frombuffer(symbols, np.uint8)
    huff = torch.from_numpy(huff).to(dev)
    want = ops.jpeg_transform(torch.from_numpy(x_host).to(dev), quality, hs, vs)
    first = [k for k, sc in enumerate(script) if sc[3] == 0]
    whole = -(-8 * max(len(s) for s in segments) // 32) * 32
    out = []
    for subseq_bits in (256, 512, 1024, 2048, whole):
        size = int(ops._lib.load().nimg_jpeg_decode_progressive_workspace_bytes(n, h, w, hs, vs, 0, len(script), ecd.numel(), subseq_bits))
        ws = torch.empty(size, dtype=torch.uint8, device=dev)

        def decode():
            return ops.jpeg_decode_progressive(ecd, off, huff, rows6, h, w, hs, vs, subseq_bits=subseq_bits, workspace=ws)
        ms = {}
        ms['decode_progressive'], (coef, status, rounds) = timed(decode, reps)
        assert int(status.abs().sum()) == 0 and torch.equal(coef, want)
        ms['decode_batch_progressive'], yp = timed(
            lambda: jpeg_helpers.decode_batch(files, subseq_bits=subseq_bits, allow_progressive=True), max(3, reps // 4))
        ms['decode_batch_baseline_twins'], yb = timed(lambda: jpeg_helpers.decode_batch(twins, subseq_bits=subseq_bits), max(3, reps // 4))
        assert np.array_equal(yp, yb)
        r = rounds.cpu().numpy()[:, first]
        out.append({'mode': 'decode_progressive', 'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality,
                    'subseq_bits': subseq_bits, 'sequential': subseq_bits == whole, 'segment_bytes': int(ecd.numel()),
                    'baseline_bytes': sum(len(f) for f in twins), 'progressive_bytes': sum(len(f) for f in files), 'workspace_bytes': size,
                    'rounds': {'min': int(r.min()), 'median': float(np.median(r)), 'max': int(r.max())},
                    'rounds_per_scan_max': r.max(axis=0).tolist(),
                    'ms': {k: round(v, 4) for k, v in ms.items()}, 'kernel_ms': kernel_ms(decode, reps, PROGRESSIVE_STAGES),
                    'images_per_s': {k: n / v * 1e3 for k, v in ms.items()}})
    return out


def measure_optimize(x_host, quality, subsampling, reps, dev):
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x_host.shape
    lib = ops._lib.load()
    coef = ops.jpeg_transform(torch.from_numpy(x_host).to(dev), quality, hs, vs)
    ws = torch.empty(ops.jpeg_workspace_bytes(n, h, w, hs, vs), dtype=torch.uint8, device=dev)
    ws_t = torch.empty(int(lib.nimg_jpeg_encode_tables_workspace_bytes(n, h, w, hs, vs)), dtype=torch.uint8, device=dev)
    out = torch.empty(n * (192 * ops.jpeg_geometry(h, w, hs, vs)[1] + 1024), dtype=torch.uint8, device=dev)
    hist = torch.empty((n, 4, 257), dtype=torch.int32, device=dev)
    ms = {}
    ms['encode'], (_, base) = timed(lambda: ops.jpeg_encode(coef, h, w, hs, vs, out=out, workspace=ws), reps)
    base = base.cpu().numpy().astype(np.int64)
    ms['histogram'], _ = timed(lambda: ops.jpeg_histogram(coef, h, w, hs, vs, out=hist), reps)
    ms['optimal_tables'], (tables, tstatus) = timed(lambda: ops.jpeg_optimal_tables(hist), reps)
    ms['encode_tables'], (_, lengths, status) = timed(lambda: ops.jpeg_encode_tables(coef, tables, h, w, hs, vs, out=out, workspace=ws_t), reps)
    assert int(tstatus.abs().sum()) == 0 and int(status.abs().sum()) == 0
    lengths = lengths.cpu().numpy().astype(np.int64)
    ms['encode_batch_total'], plain = timed(lambda: jpeg_helpers.encode_batch(x_host, quality, subsampling), max(3, reps // 4))
    ms['encode_batch_optimize_total'], files = timed(lambda: jpeg_helpers.encode_batch(x_host, quality, subsampling, optimize=True), max(3, reps // 4))
    assert [len(f) for f in plain] == (base + jpeg_helpers.JPEG_HEADER_BYTES + 2).tolist()
    heads = jpeg_helpers._header_lengths(h, w, quality, subsampling, n, tables.cpu().numpy(), None, 0, False)
    assert [len(f) for f in files] == (lengths + heads + 2).tolist()
    return {'mode': 'optimize', 'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality,
            'segment_bytes': int(base.sum()), 'segment_bytes_optimize': int(lengths.sum()),
            'file_bytes': int(sum(len(f) for f in plain)), 'file_bytes_optimize': int(sum(len(f) for f in files)),
            'workspace_bytes': ws.numel(), 'workspace_bytes_tables': ws_t.numel(),
            'ms': {k: round(v, 4) for k, v in ms.items()}, 'images_per_s': {k: n / v * 1e3 for k, v in ms.items()}}


def measure_progressive(x_host, quality, subsampling, reps, dev):
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x_host.shape
    lib = ops._lib.load()
    coef = ops.jpeg_transform(torch.from_numpy(x_host).to(dev), quality, hs, vs)
    ws_t = torch.empty(int(lib.nimg_jpeg_encode_tables_workspace_bytes(n, h, w, hs, vs)), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(int(lib.nimg_jpeg_progressive_workspace_bytes(n, h, w, hs, vs, 0)), dtype=torch.uint8, device=dev)
    out = torch.empty(n * (192 * ops.jpeg_geometry(h, w, hs, vs)[1] + 1024), dtype=torch.uint8, device=dev)
    hist = torch.empty((n, 10, 257), dtype=torch.int32, device=dev)
    tables4 = ops.jpeg_optimal_tables(ops.jpeg_histogram(coef, h, w, hs, vs))[0]
    ms = {}
    ms['encode_tables'], _ = timed(lambda: ops.jpeg_encode_tables(coef, tables4, h, w, hs, vs, out=out, workspace=ws_t), reps)
    ms['progressive_histogram'], _ = timed(lambda: ops.jpeg_progressive_histogram(coef, h, w, hs, vs, out=hist), reps)
    ms['optimal_tables'], (tables, tstatus) = timed(lambda: ops.jpeg_optimal_tables(hist), reps)
    ms['encode_progressive'], (_, lengths, status) = timed(
        lambda: ops.jpeg_encode_progressive(coef, tables, h, w, hs, vs, out=out, workspace=ws_p), reps)
    assert int(tstatus.abs().sum()) == 0 and int(status.abs().sum()) == 0
    lengths = lengths.cpu().numpy().astype(np.int64)
    plain = jpeg_helpers.encode_batch(x_host, quality, subsampling)
    ms['encode_batch_optimize_total'], optimised = timed(lambda: jpeg_helpers.encode_batch(x_host, quality, subsampling, optimize=True), max(3, reps // 4))
    ms['encode_batch_progressive_total'], files = timed(lambda: jpeg_helpers.encode_batch(x_host, quality, subsampling, progressive=True), max(3, reps // 4))
    assert sum(len(f) for f in files) - int(lengths.sum()) == sum(
        sum(len(p) for p in jpeg_helpers.jpeg_progressive_pieces(h, w, quality, subsampling, t)) + 2 for t in tables.cpu().numpy())
    return {'mode': 'progressive', 'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality,
            'segment_bytes_progressive': int(lengths.sum()), 'file_bytes': int(sum(len(f) for f in plain)),
            'file_bytes_optimize': int(sum(len(f) for f in optimised)), 'file_bytes_progressive': int(sum(len(f) for f in files)),
            'workspace_bytes_tables': ws_t.numel(), 'workspace_bytes_progressive': ws_p.numel(),
            'ms': {k: round(v, 4) for k, v in ms.items()}, 'images_per_s': {k: n / v * 1e3 for k, v in ms.items()}}


def measure_qtables(x_host, quality, subsampling, reps, dev):
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x_host.shape
    x = torch.from_numpy(x_host).to(dev)
    pair = np.stack([jpeg_helpers.libjpeg_qtable(quality, c).ravel() for c in (0, 1)])
    qt = jpeg_helpers._device_tables(jpeg_helpers.check_qtables(pair)[None], n, dev)
    ws = torch.empty(ops.jpeg_workspace_bytes(n, h, w, hs, vs), dtype=torch.uint8, device=dev)
    out = torch.empty(n * (192 * ops.jpeg_geometry(h, w, hs, vs)[1] + 1024), dtype=torch.uint8, device=dev)
    ms = {}
    ms['transform'], (coef, err) = timed(lambda: ops.jpeg_transform_tables(x, qt, hs, vs, workspace=ws), reps)
    assert int(err.item()) == 0 and torch.equal(coef, ops.jpeg_transform(x, quality, hs, vs))
    ms['encode'], (data, lengths) = timed(lambda: ops.jpeg_encode(coef, h, w, hs, vs, out=out, workspace=ws), reps)
    ln = lengths.cpu().numpy().astype(np.int64)
    ms['reconstruct'], y = timed(lambda: ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs, workspace=ws), reps)
    ms['compress_batch_total'], (yb, sizes) = timed(
        lambda: jpeg_helpers.compress_batch(x_host, None, subsampling=subsampling, qtables=pair), reps)
    assert np.array_equal(yb, y.cpu().numpy()) and sizes == (ln + jpeg_helpers.JPEG_HEADER_BYTES + 2).tolist()
    return {'mode': 'qtables', 'subsampling': subsampling, 'batch': n, 'size': [h, w], 'quality': quality, 'bytes': int(ln.sum()),
            'bpp': 8.0 * float(np.mean(sizes)) / h / w, 'ms': {k: round(v, 4) for k, v in ms.items()},
            'images_per_s': {k: n / v * 1e3 for k, v in ms.items()}}


def pillow(x_host, quality, subsampling, reps):
    from PIL import Image
    u8 = np.clip(np.trunc(np.float32(255) * x_host), 0, 255).astype(np.uint8)
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        for img in u8:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling=0 if subsampling == '4:4:4' else 2)
            np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        times.append((time.perf_counter() - t) * 1e3)
    return {'subsampling': subsampling, 'batch': len(u8), 'pillow_ms': round(float(np.median(times)), 3),
            'pillow_images_per_s': len(u8) / float(np.median(times)) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--quality', type=int, default=75)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--pillow', action='store_true', help='time Pillow on the host instead (no GPU needed)')
    ap.add_argument('--decode', action='store_true', help='time the decoder instead, per subseq_bits setting')
    ap.add_argument('--decode-progressive', action='store_true', help='time reading progressive files, per subseq_bits setting')
    ap.add_argument('--optimize', action='store_true', help='time writing with optimised Huffman tables next to nimg_jpeg_encode')
    ap.add_argument('--progressive', action='store_true', help='time writing progressive files next to nimg_jpeg_encode_tables')
    ap.add_argument('--qtables', action='store_true', help="time the table form with libjpeg's tables of --quality instead")
    ap.add_argument('--restart', type=int, default=0, help='restart interval in MCUs of the files written and read (default mode, --decode)')
    ap.add_argument('--restart-rows', type=int, default=0, help='the same in MCU rows: the interval follows the sub-sampling')
    args = ap.parse_args()
    x = natural_images(args.batch, args.size, args.size, seed=1)
    if args.pillow:
        for subsampling in SUBSAMPLINGS:
            print(json.dumps(pillow(x, args.quality, subsampling, max(3, args.reps // 4))))
        return
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_time.py needs a GPU (or --pillow)')
    dev = torch.device('cuda', 0)
    if args.decode:
        for subsampling in SUBSAMPLINGS:
            ri = interval_of(args, args.size, args.size, subsampling)
            measure_decode(x[:4], args.quality, subsampling, 2, dev, ri)              # warm-up
            for row in measure_decode(x, args.quality, subsampling, args.reps, dev, ri):
                print(json.dumps(dict(row, csrc_sha16=csrc_sha16())), flush=True)
        return
    if args.decode_progressive:
        for subsampling in SUBSAMPLINGS:
            measure_decode_progressive(x[:4], args.quality, subsampling, 2, dev)      # warm-up
            for row in measure_decode_progressive(x, args.quality, subsampling, args.reps, dev):
                print(json.dumps(dict(row, csrc_sha16=csrc_sha16())), flush=True)
        return
    if args.optimize:
        for subsampling in SUBSAMPLINGS:
            measure_optimize(x[:4], args.quality, subsampling, 2, dev)                # warm-up
            print(json.dumps(dict(measure_optimize(x, args.quality, subsampling, args.reps, dev), csrc_sha16=csrc_sha16())), flush=True)
        return
    if args.progressive:
        for subsampling in SUBSAMPLINGS:
            measure_progressive(x[:4], args.quality, subsampling, 2, dev)             # warm-up
            print(json.dumps(dict(measure_progressive(x, args.quality, subsampling, args.reps, dev), csrc_sha16=csrc_sha16())), flush=True)
        return
    if args.qtables:
        for subsampling in SUBSAMPLINGS:
            measure_qtables(x, args.quality, subsampling, 3, dev)            # warm-up
            print(json.dumps(dict(measure_qtables(x, args.quality, subsampling, args.reps, dev), csrc_sha16=csrc_sha16())), flush=True)
        return
    for subsampling in SUBSAMPLINGS:
        ri = interval_of(args, args.size, args.size, subsampling)
        measure(x, args.quality, subsampling, 3, dev, ri)                # warm-up: code objects, allocator
        print(json.dumps(dict(measure(x, args.quality, subsampling, args.reps, dev, ri), csrc_sha16=csrc_sha16())))


if __name__ == '__main__':
    main()
