#!/usr/bin/env python3
"""
bench.py - raw patches/s (forward + backward + Adam) of the imaging channel  UNet ISP -> manipulations -> codec -> FAN
at 256x256 RGB (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--workload c4|c2|c3|c5] [--dump-outputs DIR] [--full]

N > 1 without a torch.distributed environment: bench.py re-launches itself as
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`
(one rank per GPU over RCCL); under an existing launcher (RANK / WORLD_SIZE set) it just joins the group.

Workloads (BASELINE.json configs):
  c4 (default, configs[3], the configuration the metric is quoted on): B = 64 raw patches / GPU -> UNet -> (5B,256,256,3)
      [native, sharpen:1, resample:50, gaussian:0.83, jpeg:80] -> dJPEG(80, soft) -> FAN -> CE + 0.1 mse255 -> backward to the
      UNet and FAN weights -> gradient all-reduce (N > 1) -> Keras Adam.  Unit = one raw patch.
  c2 (configs[1]): train_nip.py --nip UNet - NIPModel.training_step (L2 loss on 255-scaled images, Keras Adam) on B = 32 RAW
      patches of 64x64x4 -> RGB 128x128 (training/pipeline.py:191-247, models/pipelines.py:77-90).  Unit = one raw patch.
  c3 (configs[2]): TwitterDCN-32C training step on B = 50 RGB patches of 256x256 (l2 + 250 H; the batch size train_dcn.py:102
      fixes).  Unit = one RGB patch.
  c5 (configs[4]): the full channel with the learned codec, UNet -> manipulations -> TwitterDCN-32C -> FAN, B = 16 raw
      patches / GPU (128 global on 8 GPUs), trainable nip + dcn, lambda_dcn 0.1.  Unit = one raw patch.
A "step" = one training step on a synthetic batch already resident in HBM.  Weak scaling: every rank processes its own B
units.  Rank 0 prints ONE JSON line.

Timing: W warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides (max over ranks) -> `value`,
`ms_per_step` = wall milliseconds of one timed step.  HIP events recorded between five equal blocks of the same K steps give
`config.block_ms_per_step` (their median is reported next to the contract figure; no extra host synchronisation inside the
timed region).

A plain run does only what the headline needs: set up, warm up (incl. the choice of launch path below), time the K steps,
write the outputs if asked, print the line.  --dump-outputs DIR: after the timed steps, what the timed path computed in its
last step, as DIR/<name>.npy (float32 / float64) - the values the step returned (`loss`, `loss_<part>`) and the weights of
every model it trains after its update (`<model>.<parameter>`, '/' -> '.'); a fixed, seeded sample of each if they exceed
64 MB together.  Inputs and initial weights are seeded: the same arguments give the same inputs in every run.

--full adds everything else below (each extra still subject to its own --no-* switch).  Extra objects on a --full line:
  roofline     - the workload's dominant kernel timed live with HIP events on the launch stream: algorithmic FLOPs of one
                 launch / average launch time against the dense MFMA peak of the compute dtype; traffic = HBM bytes per launch
                 from the committed PMC passes (profiles/*pmc_dominant_kernel.json: 2 x FETCH_SIZE + WRITE_SIZE, separate
                 --pmc runs), scaled to this launch's image count
  cpu_baseline - the oracle's CPU port (torch float32, 32 host threads - more only adds barrier overhead at these layer
                 sizes; the host's thread count is reported) of the SAME step on a bounded sample: 2 warm-up steps, median of
                 >= 5 timed steps
--dtype bf16 (default) = throughput mode: bf16 MFMA operands, float32 accumulation, float32 master weights / optimizer.
--dtype f32 = parity mode (exact float32 MFMA; the mode the 1e-4 parity tests run in).  At N = 1 a --full c4 run also
times parity-mode steps (top-level f32_mode_* keys, `roofline_f32`) and runs the trained-parity leg (trained_parity(): one
seeded recipe - NIP pre-training, FAN warm-up, joint training, fixed step counts - run entirely in bf16 and entirely in float32
from the same initial weights) to report accuracy / PSNR parity of the throughput mode on held-out patches.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

F32_MFMA_PEAK_TFLOPS = 157.3       # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0     # same guide: bf16 MFMA dense (the 5 PF headline includes 2:1 sparsity)
GMAC_UNET, GMAC_FAN, GMAC_DCN = 3.079, 2.705, 9.742          # SURVEY appendix A, forward, per image
MANIPS = ['sharpen:1', 'resample:50', 'gaussian:0.83', 'jpeg:80']


def synthetic_batch(b, raw_patch, seed):
    from util import bayer_from_rgb, natural_images
    rgb = natural_images(b, 2 * raw_patch, 2 * raw_patch, seed=seed)
    return bayer_from_rgb(rgb), rgb


# ----------------------------------------------------------------------------------------------------------------------
# workloads
class Workload(object):
    """build(dev, rank) -> step(); units = raw (or RGB) patches per step and rank."""
    key = name = unit_name = ''
    default_batch = 64
    gflop_per_unit = 0.0
    hbm_bytes_per_unit = None         # (bf16, f32) op-by-op compulsory traffic model, SURVEY 8d (c4 only)

    def __init__(self, args):
        self.args = args
        self.batch = args.batch or self.default_batch

    def build(self, dev, rank):
        raise NotImplementedError

    def finish(self):
        pass

    def trained_models(self):
        """[(name, model)] of every model the step updates: their weights after the last step are part of its result."""
        return []

    def step_count(self):
        """Adam's step count as the eager path keeps it."""
        raise NotImplementedError

    def flush(self):
        """Issue whatever a step left for the next one (the workflow's pipelined FAN update); a no-op otherwise."""
        wf = getattr(self, 'wf', None)
        if wf is not None and hasattr(wf, 'finish_pending'):
            wf.finish_pending()


class ChannelJPEG(Workload):
    key = 'c4'
    name = ('train_manipulation UNet->[native,sharpen:1,resample:50,gaussian:0.83,jpeg:80]->dJPEG(QF80,soft)->FAN, ds none, '
            'trainable nip+fan, lambda_nip 0.1')
    default_batch = 64
    gflop_per_unit = 2 * 3 * (GMAC_UNET + 5 * GMAC_FAN)
    hbm_bytes_per_unit = (343.8e6, 687.5e6)

    def make_flow(self, dev, nan_check='deferred'):
        from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification
        dist_cfg = {'downsampling': 'none', 'compression': 'jpeg', 'compression_params': {'quality': 80, 'codec': 'soft'}}
        return ManipulationClassification('UNet', manipulations=MANIPS, distribution=dist_cfg, trainable={'nip'},
                                          raw_patch_size=self.args.raw_patch, device=dev, nan_check=nan_check)

    def step_args(self):
        return dict(lambda_nip=0.1, learning_rate=1e-4)

    def build(self, dev, rank):
        self.wf = self.make_flow(dev)
        raw, rgb = synthetic_batch(self.batch, self.args.raw_patch, seed=1234 + rank)
        self.bx, self.by = torch.from_numpy(raw).to(dev), torch.from_numpy(rgb).to(dev)
        kw = self.step_args()
        self.eager = lambda: self.wf.training_step(self.bx, self.by, **kw)
        self.graph = False
        # (a pipelined FAN update carries work across the step boundary: such a step is not captured)
        if self.args.graph and world_size() == 1 and not getattr(self.wf, '_pipeline_fan', False):     # the data-parallel step is not captured (RCCL launches stay eager)
            from neural_imaging_amd import graphs
            self.runner = graphs.CapturedStep(self.wf, self.bx, self.by, **kw)
            self.graph = True
            return self.runner.step
        return self.eager

    def finish(self):
        self.wf.check_nan()

    def trained_models(self):
        return [('nip', self.wf.nip), ('fan', self.wf.fan)]

    def step_count(self):
        return self.wf._step

    def dominant(self, dev):
        return time_conv5_dominant(dev, 5 * self.batch)


class ChannelDCN(ChannelJPEG):
    key = 'c5'
    name = ('full channel UNet->[native,sharpen:1,resample:50,gaussian:0.83,jpeg:80]->TwitterDCN-32C->FAN, ds none, '
            'trainable nip+dcn+fan, lambda_nip 0.1, lambda_dcn 0.1')
    default_batch = 16
    gflop_per_unit = 2 * 3 * (GMAC_UNET + 5 * GMAC_FAN + 5 * GMAC_DCN)
    hbm_bytes_per_unit = None

    def make_flow(self, dev, nan_check='deferred'):
        from neural_imaging_amd.models import compression
        from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification
        codec = compression.TwitterDCN(patch_size=2 * self.args.raw_patch, n_features=32, device=dev)
        dist_cfg = {'downsampling': 'none', 'compression': 'dcn', 'compression_params': {'model': codec}}
        return ManipulationClassification('UNet', manipulations=MANIPS, distribution=dist_cfg, trainable={'nip', 'dcn'},
                                          raw_patch_size=self.args.raw_patch, device=dev, nan_check=nan_check)

    def step_args(self):
        return dict(lambda_nip=0.1, lambda_dcn=0.1, learning_rate=1e-4)

    def trained_models(self):
        return [('nip', self.wf.nip), ('dcn', self.wf.codec), ('fan', self.wf.fan)]

    def dominant(self, dev):
        return time_conv3_dominant(dev, 5 * self.batch)


class TrainDCN(Workload):
    key = 'c3'
    name = 'train_dcn TwitterDCN-32C on 256x256 RGB patches, l2_loss + 250 H, soft-codebook 5 bpf'
    default_batch = 50          # training_spec['batch_size'] of the reference's train_dcn.py:102
    gflop_per_unit = 2 * 3 * GMAC_DCN

    def build(self, dev, rank):
        from neural_imaging_amd.models import compression
        from util import natural_images
        ps = 2 * self.args.raw_patch
        self.dcn = compression.TwitterDCN(patch_size=ps, n_features=32, device=dev)
        self.x = torch.from_numpy(natural_images(self.batch, ps, ps, seed=1234 + rank)).to(dev)
        self.graph = False
        self.eager = lambda: self.dcn.training_step(self.x, learning_rate=1e-4, sync=False)
        if self.args.graph and world_size() == 1 and not os.environ.get('NIMG_C3_EAGER'):
            from neural_imaging_amd import graphs
            self.runner = graphs.CapturedModelStep(self.dcn, self.x, learning_rate=1e-4)
            self.graph = True
            return self.runner.step
        return self.eager

    def trained_models(self):
        return [('dcn', self.dcn)]

    def step_count(self):
        return self.dcn._model.step

    def dominant(self, dev):
        return time_conv3_dominant(dev, self.batch)


class TrainNIP(Workload):
    key = 'c2'
    name = 'train_nip --nip UNet, L2 loss, RAW 64x64x4 -> RGB 128x128 (batch 32 x 128 x 128)'
    default_batch = 32
    raw_patch = 64               # BASELINE.json configs[1]: 128x128 RGB patches
    gflop_per_unit = 2 * 3 * GMAC_UNET / 4

    def build(self, dev, rank):
        from neural_imaging_amd.models import pipelines
        self.nip = pipelines.UNet(patch_size=self.raw_patch, device=dev)
        raw, rgb = synthetic_batch(self.batch, self.raw_patch, seed=1234 + rank)
        self.bx, self.by = torch.from_numpy(raw).to(dev), torch.from_numpy(rgb).to(dev)
        self.graph = False
        self.eager = lambda: self.nip.training_step(self.bx, self.by, learning_rate=1e-4)
        if self.args.graph and world_size() == 1:       # ~150 launches of 5 - 40 us: eager launches are bound by the host
            from neural_imaging_amd import graphs
            self.runner = graphs.CapturedModelStep(self.nip, self.bx, self.by, learning_rate=1e-4)
            self.graph = True
            return self.runner.step
        return self.eager

    def trained_models(self):
        return [('nip', self.nip)]

    def step_count(self):
        return self.nip._model.step

    def dominant(self, dev):
        return time_unet_dominant(dev, self.batch, self.raw_patch)


def c2_psnr_parity(dev, batch, steps=400, lr=3e-4):
    """PSNR parity of the two compute modes on config 2 (BASELINE.json configs[1]: 'demosaic conv HIP kernels vs ... PSNR'): one
    UNet initialisation trained `steps` NIPModel.training_step()s on the same batches of synthetic scenes in each mode, then the
    held-out PSNR of each result in its own mode (models/pipelines.py:77-90; training/pipeline.py:191-247)."""
    import train_parity as tp
    from neural_imaging_amd import ops
    from neural_imaging_amd.models import pipelines
    rp = TrainNIP.raw_patch
    pool = tp.make_pool(512, rp, 7100, dev)
    held = tp.make_pool(256, rp, 9100, dev)
    out = {}
    for mode in ('bf16', 'f32'):
        ops.set_compute(mode)
        nip = pipelines.UNet(patch_size=rp, device=dev)
        rng = np.random.RandomState(21)
        for _ in range(steps):
            idx = torch.from_numpy(rng.choice(pool[0].shape[0], batch, replace=False)).to(dev)
            nip.training_step(pool[0][idx], pool[1][idx], learning_rate=lr)
        mse = 0.0
        for i in range(0, held[0].shape[0], 64):
            y = nip.process(held[0][i:i + 64]).t.float()
            mse += float(((y - held[1][i:i + 64]) ** 2).mean().item()) / (held[0].shape[0] // 64)
        out[mode] = float(10 * np.log10(1.0 / mse))
        del nip
    return out


def world_size():
    return int(os.environ.get('WORLD_SIZE', '1'))


WORKLOADS = {w.key: w for w in (ChannelJPEG, TrainNIP, TrainDCN, ChannelDCN)}


# ----------------------------------------------------------------------------------------------------------------------
# dominant kernels (roofline)
def _event_time(run, reps):
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _power_under(run, ms_per_launch, seconds=0.6):
    """Socket power and shader clock WHILE the dominant kernel runs back to back for ~`seconds` (tools/ring_power.Sampler: amdsmi
    gpu_metrics at ~5 ms cadence, sysfs hwmon as a fall-back): the roofline fraction of a bf16 MFMA kernel on this part is bounded
    by the board's power limit, not by pipe occupancy (profiles/r05_ring_power.txt) - the line says how close to the cap this run
    was.  None where no power interface is readable."""
    try:
        from ring_power import Sampler
        smp = Sampler()
        if smp.smi is None and not smp.hwmon:
            return None
        n = max(200, int(seconds * 1e3 / max(ms_per_launch, 1e-3)))
        torch.cuda.synchronize()
        smp.start()
        t0 = time.perf_counter()
        ev = None
        for i in range(n):
            run()
            if (i + 1) % 400 == 0:                       # bound the launch queue (allocator), never drain it
                if ev is not None:
                    ev.synchronize()
                ev = torch.cuda.Event()
                ev.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        smp.stop_flag = True
        smp.join()
        load = [x for x in smp.samples if t0 + 0.15 <= x['t'] <= t1 - 0.02]
        pw = [x['current_socket_power'] for x in load if isinstance(x.get('current_socket_power'), (int, float)) and 0 < x['current_socket_power'] < 5000]
        if not pw:
            pw = [x[k] * 1e-6 for x in load for k in ('power1_input', 'power1_average') if isinstance(x.get(k), int) and x[k] > 0]
        ck = []
        for x in load:
            c = [v for v in (x.get('current_gfxclks') or []) if isinstance(v, (int, float)) and 0 < v < 10000]
            if c:
                ck.append(sum(c) / len(c))
        cap = None
        pc = smp.info.get('power_cap', {})
        for k in ('power_cap', 'default_power_cap', 'max_power_cap'):
            if isinstance(pc.get(k), int) and pc[k] > 0:
                cap = pc[k] / (1e6 if pc[k] > 100000 else 1.0)
                break
        out = {'launches': n, 'samples': len(load), 'ms_per_launch_sustained': 1e3 * (t1 - t0) / n,
               'socket_power_w_mean': sum(pw) / len(pw) if pw else None, 'power_cap_w': cap,
               'gfx_clock_mhz_mean': sum(ck) / len(ck) if ck else None, 'gfx_clock_mhz_max': 2400}
        if pw and cap:
            out['frac_of_power_cap'] = out['socket_power_w_mean'] / cap
        return out
    except Exception as e:                                 # noqa: a measurement extra must never take the bench line down
        return {'error': repr(e)[:200]}


def _pmc_traffic(fname, key, n, stamped=False):
    """HBM bytes per launch from a committed counter profile (rocprofv3 --pmc, separate FETCH_SIZE / WRITE_SIZE passes, see
    profiles/README.md), scaled to n images.  stamped: the file carries the hash of the kernel sources it was taken on
    (tools/src_stamp.py) and is used only if that equals the sources of this run -> (bytes or None, source record)."""
    path = os.path.join(ROOT, 'profiles', fname)
    if stamped:
        from src_stamp import load_if_current
        data, src = load_if_current(path)
        if data is None:
            return None, src
        try:
            return data[key]['traffic_bytes_per_launch'] * n / data[key]['images'], src
        except KeyError:
            return None, dict(src, status='no entry ' + key)
    try:
        with open(path) as f:
            pmc = json.load(f)[key]
        return pmc['traffic_bytes_per_launch'] * n / pmc['images'], {'file': 'profiles/' + fname, 'status': 'unstamped'}
    except (OSError, KeyError, ValueError):
        return None, {'file': 'profiles/' + fname, 'status': 'missing'}


PMC_RING = 'r06_pmc_ring_kernel.json'            # tools/pmc_ring.sh on the final build of the round
PMC_STEP = 'r06_pmc_step_total.json'             # tools/pmc_step_total.py, same


def time_conv5_dominant(dev, n, reps=20):
    """FAN conv3 forward (5x5, 64 -> 128 @ 64x64, the 839 MMAC/image layer) - one launch, HIP events on the stream it runs
    on (the kernels are launched on torch's current stream, so torch.cuda.Event brackets them)."""
    from neural_imaging_amd import ops
    x = torch.randn((n, 64, 64, 64), device=dev)
    stored_bf16 = ops.COMPUTE == 'bf16' and ops.STORE_BF16
    if stored_bf16:                   # the FAN's pooled activations live in HBM as bf16 in throughput mode
        x = x.to(torch.bfloat16)
    w = torch.randn((5, 5, 64, 128), device=dev) * 0.05
    b = torch.zeros((128,), device=dev)
    out = torch.empty((n, 64, 64, 128), device=dev)
    # throughput mode: the op exactly as the FAN runs it - convolution + LeakyReLU + 2x2 max-pool in one kernel, bf16
    # pooled output + arg-max bytes (same kernel, same FLOPs; only the epilogue's store volume differs from the plain call)
    run = (lambda: ops.conv2d_pool(x, w, b, out_bf16=True)) if stored_bf16 else \
        (lambda: ops.conv2d(x, w, b, act='leaky_relu', out=out))
    ms = _event_time(run, reps)
    power = _power_under(run, ms) if stored_bf16 else None
    flops = 2.0 * 25 * 64 * 128 * 64 * 64 * n
    kname = 'conv_fwd_kernel<5,1,16,16,1,64,8>' if ops.COMPUTE == 'f32' else (
        'conv5_ring_kernel<128>' if stored_bf16 else 'conv_fwd_bf16_kernel<5,1,16,16,1,64>')
    traffic, tsrc = _pmc_traffic(PMC_RING, 'bf16_stored_input_pooled', n, stamped=True) if stored_bf16 else \
        _pmc_traffic('r01_pmc_dominant_kernel.json', ops.COMPUTE, n)
    return {'kernel': kname + ' (FAN conv3 fwd{}, {}x64x64x64->128)'.format(' + LReLU + pool' if stored_bf16 else '', n),
            'traffic': traffic, 'traffic_source': tsrc, 'flops_per_launch': flops, 'ms_per_launch': ms, 'tflops': flops / (ms * 1e-3) / 1e12,
            'power': power}


def time_conv3_dominant(dev, n, reps=20):
    """TwitterDCN residual-block convolution (3x3, 128 -> 128 @ 64x64; 12 of them = 7.2 of the 9.74 GMAC per image)."""
    from neural_imaging_amd import ops
    x = torch.randn((n, 64, 64, 128), device=dev)
    w = torch.randn((3, 3, 128, 128), device=dev) * 0.05
    b = torch.zeros((128,), device=dev)
    out = torch.empty((n, 64, 64, 128), device=dev)
    ms = _event_time(lambda: ops.conv2d(x, w, b, act='leaky_relu', out=out), reps)
    flops = 2.0 * 9 * 128 * 128 * 64 * 64 * n
    kname = 'conv_fwd_kernel<3,1,...>' if ops.COMPUTE == 'f32' else 'conv_fwd_bf16_kernel<3,1,16,16,1,64>'
    traffic, tsrc = _pmc_traffic('r02_pmc_dcn_kernel.json', ops.COMPUTE, n)
    return {'kernel': kname + ' (TwitterDCN residual conv fwd, {}x64x64x128->128)'.format(n), 'traffic': traffic,
            'traffic_source': tsrc,
            'flops_per_launch': flops, 'ms_per_launch': ms, 'tflops': flops / (ms * 1e-3) / 1e12}


def time_unet_dominant(dev, n, raw_patch, reps=20):
    """UNet dc41 (3x3, concat(32 + 32) -> 32 at the RAW resolution: 302 of the 3079 MMAC per patch, the largest layer of the
    ISP), as the model runs it in throughput mode: two bf16-stored inputs, bf16 output."""
    from neural_imaging_amd import ops
    h = raw_patch
    stored_bf16 = ops.COMPUTE == 'bf16' and ops.STORE_BF16
    a, b2 = torch.randn((n, h, h, 32), device=dev), torch.randn((n, h, h, 32), device=dev)
    if stored_bf16:
        a, b2 = a.to(torch.bfloat16), b2.to(torch.bfloat16)
    w = torch.randn((3, 3, 64, 32), device=dev) * 0.05
    b = torch.zeros((32,), device=dev)
    ms = _event_time(lambda: ops.conv2d(a, w, b, act='leaky_relu', x2=b2, out_bf16=stored_bf16), reps)
    flops = 2.0 * 9 * 64 * 32 * h * h * n
    return {'kernel': 'conv_fwd_{}kernel<3,1,16,16,1,32> (UNet dc41 fwd, {}x{}x{}x(32+32)->32)'.format(
                'bf16_' if ops.COMPUTE == 'bf16' else '', n, h, h),
            'traffic': None, 'traffic_source': None, 'flops_per_launch': flops, 'ms_per_launch': ms,
            'tflops': flops / (ms * 1e-3) / 1e12}


# ----------------------------------------------------------------------------------------------------------------------
# CPU baseline (oracle port, child process)
def _host_cpu():
    model = None
    try:
        with open('/proc/cpuinfo') as f:
            for ln in f:
                if ln.startswith('model name'):
                    model = ln.split(':', 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    return model, os.cpu_count() or usable, usable


def cpu_baseline_worker(workload, raw_patch, budget_s):
    """Oracle port on the host cores: torch float32 CPU, the same step, bounded to ~budget_s of timed work."""
    from oracle import nets as onets, workflow as owf
    from util import natural_images
    model, total, usable = _host_cpu()
    # 32 threads: the box offers 256 hardware threads, but the layers of a B = 2 step are far too small for them - with
    # torch.set_num_threads(256) one step did not finish in 240 s (oneDNN barrier overhead), with 32 it takes ~0.5 s
    usable = max(1, min(usable, 32))
    torch.set_num_threads(usable)
    b = 2
    if workload == 'c3':
        dcn = onets.dcn_init(777, dtype=torch.float32)
        x = torch.from_numpy(natural_images(b, 2 * raw_patch, 2 * raw_patch, seed=99))
        trainer = onets.DCNTrainer(dcn)
        step = lambda: trainer.training_step(x, learning_rate=1e-4)
    elif workload == 'c2':                  # NIPModel.training_step restated: tape over mse255(UNet(x), y), Keras Adam
        from oracle import tfops as T
        b = 8
        p = onets.unet_init(1234, dtype=torch.float32)
        ps = list(p.values())
        raw, rgb = synthetic_batch(b, raw_patch, seed=99)
        bx, by = torch.from_numpy(raw), torch.from_numpy(rgb)
        state = {'t': 0, 'm': [torch.zeros_like(q) for q in ps], 'v': [torch.zeros_like(q) for q in ps]}

        def step():
            for q in ps:
                q.requires_grad_(True)
            grads = torch.autograd.grad(T.mse255(onets.unet_forward(p, bx), by), ps)
            for q in ps:
                q.requires_grad_(False)
            state['t'] += 1
            with torch.no_grad():
                T.adam_step(ps, list(grads), state['m'], state['v'], state['t'], 1e-4)
    else:
        # the channel step at TWO operating points (B = 2 on 32 threads alone is an undersized CPU step):
        # B = 2 / 32 threads and B = 8 / 64 threads; `value` is the better of the two, both are reported in `variants`
        kw = dict(lambda_nip=0.1, learning_rate=1e-4)
        variants = []
        for b, threads in ((2, 32), (8, 64)):
            threads = max(1, min(len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else total, threads))
            torch.set_num_threads(threads)
            if workload == 'c5':
                wf = owf.Workflow(trainable=('nip', 'dcn'), codec='dcn', dtype=torch.float32)
                kw['lambda_dcn'] = 0.1
            else:
                wf = owf.Workflow(trainable=('nip',), jpeg_quality=80, dtype=torch.float32)
            raw, rgb = synthetic_batch(b, raw_patch, seed=99)
            bx, by = torch.from_numpy(raw), torch.from_numpy(rgb)
            step = lambda: wf.training_step(bx, by, **kw)
            t_var = time.time()
            step()                                                              # warm-up
            if b == 2:
                step()
            times = []
            while len(times) < 3 or (len(times) < 12 and time.time() - t_var < 0.5 * budget_s):
                t0 = time.time()
                step()
                times.append(time.time() - t0)
            variants.append({'batch': b, 'threads': threads, 'steps': len(times), 'value': b / float(np.median(times))})
        best = max(variants, key=lambda v: v['value'])
        return {'value': best['value'], 'unit': 'patches/s', 'cores': best['threads'], 'kind': 'port', 'host_cores': total,
                'cpu_model': model, 'variants': variants,
                'sample': 'better of two operating points (median step after warm-up): ' + '; '.join(
                    'B={} on {} threads: {:.2f} patches/s over {} steps'.format(v['batch'], v['threads'], v['value'], v['steps'])
                    for v in variants) + ' - raw {0}x{0}x4 patches, torch-CPU float32 restatement of the same step (restated-'
                    'reference CPU baseline, TF2 unavailable), {1} host threads'.format(raw_patch, total)}
    for _ in range(2):                                                      # warm-up
        step()
    times, t_all = [], time.time()
    while len(times) < 5 or (len(times) < 15 and time.time() - t_all < budget_s):
        t0 = time.time()
        step()
        times.append(time.time() - t0)
    med = float(np.median(times))
    return {'value': b / med, 'unit': 'patches/s', 'cores': usable, 'kind': 'port', 'host_cores': total, 'cpu_model': model,
            'sample': 'median of {} step(s) after 2 warm-ups, B={} {} patches, torch-CPU float32 restatement of the same step '
                      '(restated-reference CPU baseline, TF2 unavailable), {} threads of {} host threads'.format(
                          len(times), b, 'RGB 256x256' if workload == 'c3' else 'raw {0}x{0}x4'.format(raw_patch), usable, total)}


def cpu_baseline(workload, raw_patch, budget_s=20.0, hard_timeout_s=150):
    """Run the CPU leg in a child process so a badly provisioned host can never stall the GPU measurement."""
    _, total, usable = _host_cpu()
    fail = {'value': None, 'unit': 'patches/s', 'cores': min(usable, 32), 'kind': 'port', 'host_cores': total}
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-baseline-worker', '--workload', workload,
                              '--raw-patch', str(raw_patch), '--cpu-budget', str(budget_s)], capture_output=True, text=True,
                             timeout=hard_timeout_s, env=dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='',
                                                           OMP_NUM_THREADS=str(min(usable, 32))))
        for ln in reversed(out.stdout.strip().splitlines()):
            if ln.startswith('{'):
                return json.loads(ln)
        return dict(fail, sample='cpu worker failed: ' + out.stderr[-200:])
    except subprocess.TimeoutExpired:
        return dict(fail, sample='cpu worker exceeded {} s'.format(hard_timeout_s))


# ----------------------------------------------------------------------------------------------------------------------
def self_launch(args):
    """--gpus N without a launcher environment: start N ranks under torch.distributed.run and relay their output."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '4')
    return subprocess.call(cmd, env=env)


def dp1_nccl_leg(wl, n=20):
    """Eager C4 steps with the data-parallel path live on ONE rank: `nccl` (= RCCL) process group of world size 1,
    parallel.force_collectives() -> the FAN / UNet-decoder / UNet-encoder gradient buckets are launched as asynchronous
    all-reduces while the backward pass continues, the NaN flag is MAX-reduced, Adam waits for the buckets.  Reported next to
    the plain eager step timed the same way in the same process."""
    from neural_imaging_amd import parallel
    from neural_imaging_amd.graphs import RunAhead
    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t, host = time.perf_counter(), 0.0
        pace = RunAhead()
        for _ in range(n):
            c = time.thread_time()
            fn()
            host += 1e3 * (time.thread_time() - c) / n       # issuing the step only: the pacing wait below spins on an event
            pace()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / n, host
    plain_ms, plain_host = timed(wl.eager)
    parallel.force_collectives(True)
    try:
        parallel.init_from_env('nccl')
        assert parallel.is_distributed() and torch.distributed.get_backend() == 'nccl'
        dp_ms, dp_host = timed(wl.eager)
        wl.wf.check_nan()
    finally:
        parallel.force_collectives(False)
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
    return {'dp1_nccl_ms_per_step': dp_ms, 'dp1_nccl_host_cpu_ms_per_step': dp_host,
            'dp1_plain_eager_ms_per_step': plain_ms, 'dp1_plain_eager_host_cpu_ms_per_step': plain_host}


def trained_parity(wl, dev, pre, warm, joint, joint_lr=5e-5):
    """PSNR / accuracy parity of the throughput mode on a channel that has LEARNED, at the workload's own scale (BASELINE.json
    "PSNR/acc parity").  FIXED protocol, no checkpoint selection: the same seeded recipe is run twice from
    identical initial weights on identical batches - once entirely in bf16 throughput mode, once entirely in float32 parity
    mode - and the two TRAINED channels are compared on 256 held-out patches:
        1. NIP pre-training alone on its L2 loss (train_nip.py -> training/pipeline.py): `pre` steps, lr 3e-4;
        2. FAN warm-up with the NIP frozen (train_manipulation.py without `--train nip`): `warm` steps, lr 1e-4 (the reference's
           default, training/manipulation.py:28);
        3. joint optimisation (lambda_nip 0.1, `--train nip`): `joint` steps at lr `joint_lr`.
    Why 5e-5 and not the reference's 1e-4 for step 3: with Keras' cross-entropy on clipped probabilities (eager mode:
    clip_by_value(p, 1e-7, 1 - 1e-7), zero gradient outside) one large Adam step can push a whole class under the clip, where its
    gradient is exactly zero FOR EVER - CE jumps to ~3.6 (= 16.1 / 5 + the rest), that class reads 0.0.  On these synthetic scenes
    at lr 1e-4 that happens in 4 of 8 runs between joint steps 50 and 800, in float32 exactly as in bf16 (profiles/
    r06_parity_rootcause.txt: rounds 3 - 5 quoted a checkpoint that sat before / inside / behind such an event; not a kernel
    regression); at 5e-5 and 3e-5 in 0 of 16 runs.
    Reported: each trained channel in its own mode (accuracy, per-class accuracy, CE, ISP PSNR), their deltas, the share of
    identical decisions of the two trained channels, and the cross evaluation (each set of weights through the OTHER kernel set:
    inference parity at one checkpoint).  C4's classes 'native' and 'jpeg:80' are the same image after the channel's own
    dJPEG(80) (recompression at one quality is idempotent up to rounding): 0.8 is the accuracy ceiling, those two decisions are
    coin flips, and the per-class floor is therefore checked with the two merged (`first_or_last_class_accuracy`)."""
    import train_parity as tp
    from neural_imaging_amd import ops
    b, rp = wl.batch, wl.args.raw_patch
    pool = tp.make_pool(512, rp, 7000, dev)
    held = tp.make_pool(256, rp, 9000, dev)
    wfs, secs = {}, {}
    for mode in ('bf16', 'f32'):
        t0 = time.time()
        ops.set_compute(mode)
        wf = tp.make_flow(dev, rp)                      # seeded: both modes start from the same weights
        tp.pretrain_nip(wf, pool, pre, 3e-4, b, seed=11)
        if warm > 0:
            wf._trainable.discard('nip')
            tp.train_joint(wf, pool, warm, 1e-4, b, seed=112)
            wf._trainable.add('nip')
        tp.train_joint(wf, pool, joint, joint_lr, b, seed=12)
        torch.cuda.synchronize()
        wfs[mode], secs[mode] = wf, round(time.time() - t0, 1)
    res = tp.compare(wfs, held, b)
    ops.set_compute('bf16')
    floor = lambda ev: min(ev['per_class_accuracy'][1:-1] + [ev['first_or_last_class_accuracy']])
    out = {'recipe': {'nip_pretraining_steps': pre, 'nip_pretraining_lr': 3e-4, 'fan_warmup_steps': warm, 'fan_warmup_lr': 1e-4,
                      'joint_steps': joint, 'joint_lr': joint_lr, 'lambda_nip': 0.1, 'batch': b, 'training_pool': 512,
                      'held_out_patches': 256, 'data': 'tests/util.scene_images (synthetic scenes)',
                      'protocol': 'fixed step counts, no checkpoint selection; both modes trained from one seed',
                      'training_seconds': secs},
           'trained_in_bf16': res['bf16'], 'trained_in_f32': res['f32'],
           'fan_accuracy_delta': res['fan_accuracy_delta'], 'isp_psnr_delta_db': res['isp_psnr_delta_db'],
           'decision_agreement_of_the_two_trained_channels': res['decision_agreement_of_the_two_trained_channels'],
           'worst_class_accuracy_bf16': floor(res['bf16']), 'worst_class_accuracy_f32': floor(res['f32']),
           'bf16_weights_in_f32_mode': res['bf16_weights_in_f32_mode'], 'f32_weights_in_bf16_mode': res['f32_weights_in_bf16_mode']}
    del wfs
    return out


DUMP_LIMIT_BYTES = 64 << 20


def step_outputs(wl, last):
    """What the timed path computed in its last step -> {name: float32 / float64 ndarray}: the values the step returned (the
    workflow's (loss, {'ce', 'nip', 'dcn'}), a model's loss or its dict) and the weights of every model it updated."""
    if isinstance(last, tuple):
        items = [('loss', last[0])] + [('loss_' + k, v) for k, v in last[1].items()]
    elif isinstance(last, dict):
        items = list(last.items())
    else:
        items = [('loss', last)]
    out = {}
    for name, v in items:
        if v is None or (isinstance(v, float) and np.isnan(v)):          # a part this configuration does not have
            continue
        out[name] = np.asarray(v)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for prefix, model in wl.trained_models():
        for k, v in model.state_dict().items():
            out[prefix + '.' + k.replace('/', '.').replace(':', '_')] = np.asarray(v)
    return {k: v.astype(np.float64 if v.dtype == np.float64 else np.float32) for k, v in out.items()}


def dump_outputs(arrays, out_dir, limit=DUMP_LIMIT_BYTES):
    """DIR/<name>.npy for every array; if they exceed `limit` together, a fixed seeded sample of each (sorted flat indices,
    the same share of every array)."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    rng = np.random.default_rng(20240601)
    for name in sorted(arrays):
        a = arrays[name]
        if total > limit and a.size > 1:
            keep = max(1, int(a.size * (limit - (1 << 20)) / total))     # 1 MB left for the .npy headers
            a = a.reshape(-1)[np.sort(rng.choice(a.size, keep, replace=False))]
        np.save(os.path.join(out_dir, name + '.npy'), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--workload', choices=sorted(WORKLOADS), default='c4')
    ap.add_argument('--batch', type=int, default=0, help='units per GPU per step (default: the workload\'s, c4: 64)')
    ap.add_argument('--raw-patch', type=int, default=128)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--dtype', choices=['f32', 'bf16'], default='bf16',
                    help='arithmetic type of the convolution GEMMs (bf16 = MFMA throughput mode, f32 accumulate; '
                         'f32 = parity mode)')
    ap.add_argument('--no-parity-mode', action='store_true', help='skip the float32 parity-mode legs at N=1')
    ap.add_argument('--parity-steps', type=int, default=600,
                    help='joint training steps of the trained-parity leg (0 = skip); the NIP is pre-trained for 2.5 x as many '
                         'steps first, the FAN warmed up for half as many; run once entirely in bf16 and once entirely in f32')
    ap.add_argument('--no-side-workloads', action='store_true', help='skip the short c2 / c3 / c5 runs of a --full c4 line')
    ap.add_argument('--run-ahead', type=int, default=3,
                    help='steps the launching thread may be ahead of the GPU in the timed loop (0 = unbounded), see RunAhead')
    ap.add_argument('--stall-probe', action='store_true',
                    help='diagnostic: per-step host times of the timed loop + a Python stack dump of any step that takes > 150 ms')
    ap.add_argument('--no-dp1-nccl', action='store_true', help='skip the one-rank RCCL leg (dp1_nccl_*) of a --full c4 line')
    ap.add_argument('--no-graph', dest='graph', action='store_false',
                    help='launch every kernel of the timed steps eagerly (default at N = 1: the step is ALSO captured into a HIP '
                         'graph - same kernels, same order, one launch call per step - and whichever of the two launch paths '
                         'runs the warm-up steps faster is used for the timed ones)')
    ap.add_argument('--force-graph', action='store_true', help='time the graph replay even if eager launches were faster')
    ap.add_argument('--backend', default=None, help='torch.distributed backend (default: nccl = RCCL); gloo is for a '
                                                     'functional check of the N>1 path on a one-GPU box')
    ap.add_argument('--single-device', action='store_true', help='functional check only: every rank uses cuda:0')
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline figure as well: roofline (dominant kernel, power), eager host cost, HBM '
                         'fractions, the float32 parity-mode legs, the trained-parity leg, configs 2 / 3 / 5, the one-rank RCCL '
                         'step and the CPU baseline (each still subject to its --no-* switch)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed (returned losses, updated weights) as '
                         'DIR/<name>.npy, float32 / float64, at most 64 MB in all')
    ap.add_argument('--cpu-baseline-worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--cpu-budget', type=float, default=20.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_baseline_worker:
        print(json.dumps(cpu_baseline_worker(args.workload, args.raw_patch, args.cpu_budget)))
        return
    if args.gpus > 1 and 'RANK' not in os.environ and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args))

    importlib.import_module('neural-imaging_amd')
    from neural_imaging_amd import _lib, parallel
    from neural_imaging_amd.graphs import RunAhead

    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU; there is no CPU fallback')
    if args.single_device:
        os.environ['LOCAL_RANK'] = '0'
    world = parallel.init_from_env(args.backend)
    rank = parallel.rank()
    local = int(os.environ.get('LOCAL_RANK', 0))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    _lib.load()
    from neural_imaging_amd import ops as _ops
    _ops.set_compute(args.dtype)
    if world != args.gpus:
        raise SystemExit('--gpus {} but the process group has {} rank(s)'.format(args.gpus, world))

    wl = WORKLOADS[args.workload](args)
    if getattr(wl, 'raw_patch', None):        # config 2 fixes its own patch size (128x128 RGB)
        args.raw_patch = wl.raw_patch
    step = wl.build(dev, rank)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    launch_modes = None
    if getattr(wl, 'graph', False) and hasattr(wl, 'eager') and not args.force_graph:
        # launch path: graph replay (one host call per step) or eager launches (~3 ms of host time per 9 ms step at C4).  On this
        # stack the replay of the ~165-kernel two-stream step is 3 - 5 % SLOWER than the eager launches
        # (profiles/r03_ae_graph_vs_eager.txt), on a loaded host it would be the other way round - so both are timed during the
        # warm-up (untimed part of the run) and the faster one runs the K timed steps
        launch_modes = {}
        for name, fn in (('graph', step), ('eager', wl.eager)) * 2:      # twice, alternating; the better round of each counts
            for _ in range(2):                                           # (the first eager steps after a capture re-grow scratch)
                fn()
            torch.cuda.synchronize()
            t_m = time.perf_counter()
            pace = RunAhead()
            for _ in range(max(args.warmup, 5)):
                fn()
                pace()
            torch.cuda.synchronize()
            launch_modes[name] = min(launch_modes.get(name, 1e30), 1e3 * (time.perf_counter() - t_m) / max(args.warmup, 5))
        if launch_modes['eager'] < launch_modes['graph']:
            step, wl.graph = wl.eager, False
        else:
            # a captured step counts Adam's steps itself and the eager probe steps did not advance that count: continue from
            # theirs, so that the timed steps compute the same whichever launch path won
            wl.runner.t = wl.step_count()
    nblk = 5 if args.steps >= 5 else 1
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(nblk + 1)]
    edges = [round(i * args.steps / nblk) for i in range(nblk + 1)]
    wl.flush()                                 # pipelined FAN update: nothing of the warm-up steps is carried into the timed region ...
    barrier()
    t0 = time.perf_counter()
    host_cpu = 0.0                             # CPU time this thread spends ISSUING the steps (host cost of the launch path; the
    last = None                                # run-ahead wait spins on an event and is not counted)
    host_step_ms = []
    pace = RunAhead(args.run_ahead) if args.run_ahead > 0 else (lambda: None)
    if args.stall_probe:
        import faulthandler
    for i in range(args.steps):
        if i in edges:
            marks[edges.index(i)].record()
        if args.stall_probe:
            faulthandler.dump_traceback_later(0.15, file=sys.stderr)
            t_s = time.perf_counter()
        c0 = time.thread_time()
        last = step()
        host_cpu += time.thread_time() - c0
        pace()
        if args.stall_probe:
            faulthandler.cancel_dump_traceback_later()
            host_step_ms.append(1e3 * (time.perf_counter() - t_s))
    wl.flush()                                 # ... and the last timed step's deferred part runs inside it: K whole steps
    marks[nblk].record()
    host_cpu_ms = 1e3 * host_cpu / max(args.steps, 1)
    barrier()
    dt = time.perf_counter() - t0
    wl.finish()
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:        # before any --full leg steps the model again
        dump_outputs(step_outputs(wl, last), args.dump_outputs)

    line = None
    if rank == 0:
        ms = 1e3 * dt / args.steps
        value = world * wl.batch * args.steps / dt
        blocks = [marks[i].elapsed_time(marks[i + 1]) / max(edges[i + 1] - edges[i], 1) for i in range(nblk)]
        dom = wl.dominant(dev) if args.full else None
        peak = F32_MFMA_PEAK_TFLOPS if args.dtype == 'f32' else BF16_MFMA_PEAK_TFLOPS
        if isinstance(last, tuple):
            loss = float(last[0])
        elif isinstance(last, dict):
            loss = float(last['loss'])
        else:
            loss = None
        cfg = {'workload': '{} = {}'.format(wl.key, wl.name), 'raw_patch': args.raw_patch, 'rgb_patch': 2 * args.raw_patch,
               'batch_per_gpu': wl.batch, 'global_batch': world * wl.batch, 'parallelism': 'dp%d' % world,
               'world_size': world, 'backend': torch.distributed.get_backend() if world > 1 else None,
               'hip_graph': bool(getattr(wl, 'graph', False)), 'host_cpu_ms_per_step': host_cpu_ms, 'loss': loss,
               'achieved_tflops_whole_step': value * wl.gflop_per_unit / 1e3,
               'block_ms_per_step': [round(v, 4) for v in blocks], 'median_block_ms_per_step': float(np.median(blocks))}
        if host_step_ms:
            order = np.argsort(host_step_ms)[::-1][:5]
            cfg['stall_probe_slowest_host_steps'] = [[int(j), round(host_step_ms[j], 2)] for j in order]
        if launch_modes is not None:
            cfg['launch_mode_warmup_ms_per_step'] = {k: round(v, 4) for k, v in launch_modes.items()}
        if args.full and world == 1 and getattr(wl, 'graph', False):
            # what the data-parallel step (always eager: the RCCL launches stay outside a captured graph) costs the host per
            # step: CPU time of this thread issuing 10 eager steps, and their wall time, next to the replayed figure above
            torch.cuda.synchronize()
            t_e, c_e = time.perf_counter(), time.thread_time()
            for _ in range(10):
                wl.eager()
            cfg['eager_host_cpu_ms_per_step'] = 1e2 * (time.thread_time() - c_e)
            torch.cuda.synchronize()
            cfg['eager_ms_per_step'] = 1e2 * (time.perf_counter() - t_e)
        if args.full and wl.hbm_bytes_per_unit is not None:
            # SURVEY 8d compulsory-traffic model of the whole step against 8 TB/s: one kernel per reference op
            # (343.8 MB bf16 / 687.5 MB f32 per raw patch) and the fused figure (141.9 / 283.8 MB)
            per = wl.hbm_bytes_per_unit[0 if args.dtype == 'bf16' else 1]
            cfg['hbm_frac_whole_step_op_by_op'] = value / world * per / 8e12
            cfg['hbm_frac_whole_step_fused'] = value / world * (141.9e6 if args.dtype == 'bf16' else 283.8e6) / 8e12
            if args.dtype == 'bf16' and wl.key == 'c4':
                # counter-based: HBM bytes of one step summed over ALL its dispatches (profiles/r03_pmc_step_total.json, made by
                # tools/pmc_step_total.py from separate FETCH_SIZE / WRITE_SIZE passes at B = 64) x this run's step rate
                from src_stamp import load_if_current
                data, src = load_if_current(os.path.join(ROOT, 'profiles', PMC_STEP))
                cfg['hbm_frac_whole_step_measured'] = None if data is None else \
                    value / world * data['bytes_per_raw_patch'] / 8e12
                cfg['hbm_bytes_per_raw_patch_measured'] = None if data is None else data['bytes_per_raw_patch']
                cfg['hbm_whole_step_source'] = src
        line = {
            'metric': {'c4': 'patches/s (fwd+bwd) ISP->JPEG->FAN @256^2', 'c3': 'patches/s (fwd+bwd) TwitterDCN-32C @256^2',
                       'c2': 'patches/s (fwd+bwd) UNet ISP RAW 64^2 -> RGB 128^2',
                       'c5': 'patches/s (fwd+bwd) ISP->TwitterDCN->FAN @256^2'}[wl.key],
            'value': value, 'unit': 'patches/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype,
            'data': 'synthetic (natural-image-like RAW/RGB pairs, random-init weights)', 'config': cfg,
        }
        if dom is not None:
            line['roofline'] = {'bound': 'mfma', 'achieved': dom['tflops'], 'peak': peak, 'unit': 'TFLOP/s',
                                'frac': dom['tflops'] / peak, 'traffic': dom['traffic'], 'kernel': dom['kernel'],
                                'ms_per_launch': dom['ms_per_launch'], 'flops_per_launch': dom['flops_per_launch'],
                                'traffic_source': dom.get('traffic_source'), 'power': dom.get('power')}
        if args.full and world == 1 and args.dtype == 'bf16' and not args.no_parity_mode and wl.key in ('c4', 'c5'):
            _ops.set_compute('f32')                           # same step, exact float32 MFMA (the parity-test mode), eager
            for _ in range(2):
                wl.eager()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            n32 = 5
            for _ in range(n32):
                wl.eager()
            torch.cuda.synchronize()
            dt32 = (time.perf_counter() - t1) / n32
            dom32 = wl.dominant(dev)
            line['f32_mode_patches_per_s'] = wl.batch / dt32          # top level: the driver's parser keeps flat scalars
            line['f32_mode_ms_per_step'] = 1e3 * dt32
            line['f32_mode_dominant_kernel_frac_of_peak'] = dom32['tflops'] / F32_MFMA_PEAK_TFLOPS
            _ops.set_compute(args.dtype)
            peak32 = F32_MFMA_PEAK_TFLOPS
            line['roofline_f32'] = {'bound': 'mfma', 'achieved': dom32['tflops'], 'peak': peak32, 'unit': 'TFLOP/s',
                                    'frac': dom32['tflops'] / peak32, 'traffic': dom32['traffic'], 'kernel': dom32['kernel'],
                                    'ms_per_launch': dom32['ms_per_launch'], 'flops_per_launch': dom32['flops_per_launch'],
                                    'whole_step_ms': 1e3 * dt32, 'whole_step_patches_per_s': wl.batch / dt32,
                                    'whole_step_tflops': wl.batch / dt32 * wl.gflop_per_unit / 1e3}
            if args.parity_steps > 0 and wl.key == 'c4':
                par = trained_parity(wl, dev, pre=(5 * args.parity_steps) // 2, warm=args.parity_steps // 2,
                                     joint=args.parity_steps)
                # each channel TRAINED in its own mode, evaluated in its own mode (fixed protocol)
                line['parity_fan_accuracy_bf16'] = par['trained_in_bf16']['fan_accuracy']
                line['parity_fan_accuracy_f32'] = par['trained_in_f32']['fan_accuracy']
                line['parity_isp_psnr_db_bf16'] = par['trained_in_bf16']['isp_psnr_db']
                line['parity_isp_psnr_db_f32'] = par['trained_in_f32']['isp_psnr_db']
                line['parity_worst_class_accuracy_bf16'] = par['worst_class_accuracy_bf16']
                line['parity_worst_class_accuracy_f32'] = par['worst_class_accuracy_f32']
                # one checkpoint through both kernel sets (inference parity)
                x = par['bf16_weights_in_f32_mode']
                line['parity_same_weights_fan_accuracy_delta'] = par['trained_in_bf16']['fan_accuracy'] - x['fan_accuracy']
                line['parity_same_weights_isp_psnr_delta_db'] = par['trained_in_bf16']['isp_psnr_db'] - x['isp_psnr_db']
                line['parity_same_weights_decision_agreement'] = x['decision_agreement_with_bf16_mode']
                cfg['mode_parity_after_training'] = par
                _ops.set_compute(args.dtype)
        if args.full and world == 1 and args.dtype == 'bf16' and wl.key == 'c4' and not args.no_parity_mode and \
                not args.no_side_workloads:
            # configs 2, 3 and 5 of BASELINE.json on the same line (flat scalars: the driver's parser keeps those): 30 timed steps each
            for key in ('c2', 'c3', 'c5'):
                try:
                    a2 = argparse.Namespace(**dict(vars(args), workload=key, batch=0))
                    w2 = WORKLOADS[key](a2)
                    step2 = w2.build(dev, rank)

                    def timed2(fn, n):
                        for _ in range(5):
                            fn()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        pace2 = RunAhead()
                        for _ in range(n):
                            fn()
                            pace2()
                        torch.cuda.synchronize()
                        return (time.perf_counter() - t2) / n
                    dt2 = timed2(step2, 30)
                    if getattr(w2, 'graph', False):          # both launch paths, the faster one is the figure (as for c4)
                        dt2e = timed2(w2.eager, 30)
                        line[key + '_eager_ms_per_step'] = 1e3 * dt2e
                        line[key + '_graph_ms_per_step'] = 1e3 * dt2
                        dt2 = min(dt2, dt2e)
                    w2.finish()
                    line[key + '_patches_per_s'] = w2.batch / dt2
                    line[key + '_ms_per_step'] = 1e3 * dt2
                    line[key + '_tflops'] = w2.batch / dt2 * w2.gflop_per_unit / 1e3
                    line[key + '_frac_of_mfma_peak'] = line[key + '_tflops'] / BF16_MFMA_PEAK_TFLOPS       # whole step, dense bf16 peak
                    if key == 'c2':
                        line['c2_dominant_kernel_frac_of_mfma_peak'] = w2.dominant(dev)['tflops'] / BF16_MFMA_PEAK_TFLOPS
                    del w2, step2
                except Exception as e:                       # a side figure must never take the headline line down
                    line[key + '_error'] = repr(e)[:200]
            try:                                             # config 2's "vs ... PSNR": both modes trained from one initialisation
                psnr = c2_psnr_parity(dev, TrainNIP.default_batch)
                line['c2_psnr_db_bf16'], line['c2_psnr_db_f32'] = psnr['bf16'], psnr['f32']
            except Exception as e:
                line['c2_psnr_error'] = repr(e)[:200]
            _ops.set_compute(args.dtype)
        if args.full and world == 1 and args.dtype == 'bf16' and wl.key == 'c4' and not args.no_dp1_nccl and \
                not args.no_parity_mode:
            # the data-parallel step through RCCL on this one GPU: a one-rank nccl group with the collectives
            # forced - gradient buckets, NaN-flag reduction - next to the plain eager step of the same process
            try:
                line.update(dp1_nccl_leg(wl))
            except Exception as e:
                line['dp1_nccl_error'] = repr(e)[:200]
        if args.full and not args.no_cpu_baseline and world == 1:
            line['cpu_baseline'] = cpu_baseline(wl.key, args.raw_patch)
        line['launch_path'] = 'hip_graph_replay' if cfg['hip_graph'] else 'eager_launches'
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    # RCCL writes a version banner to the C stdout of the process that created a communicator; when stdout is a file or a pipe it
    # sits in the C buffer until exit and would land BEHIND the result: drain it first, so that the JSON line is the last line
    import ctypes
    ctypes.CDLL(None).fflush(None)
    if rank == 0:
        if world > 1:
            time.sleep(0.5)                     # the other ranks drain theirs
        sys.stdout.flush()
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
