"""
Exact-arithmetic tests of the convolution kernels (throughput mode first, parity mode too).

bf16 x bf16 products are exact in float32, and float32 sums of integers are exact in any order while the sum of the absolute
terms stays below 2^24.  On small-integer operands (util.ternary / util.small_ints) every MFMA / SMFMAC / VALU kernel - whatever
its tiling, K chunks, split-K slabs or summation order - must therefore reproduce the float64 oracle (oracle.tfops) BIT FOR BIT,
and the arg-max of a pooling window (first maximum on ties) is determined exactly.  Three layers:

1. exact-integer parity (test_*_exact): np.array_equal against the oracle, every arg-max index compared.  The only inequalities
   are the two conditions on the reference that keep a case exact (util.assert_exact_conditions).
2. impulses (test_impulse_*): a one-hot weight over full-mantissa float32 x must give bf16_rne(x) shifted by that tap, a one-hot
   pixel must give bf16_rne(w) flipped around it - how operands are rounded and where each tap lands.  Equality.
3. full-mantissa operands rounded to bf16 first (test_full_mantissa_*), float64 oracle on the same values: float32 outputs
   max|got - ref| <= 2e-5 max|ref|, bf16 outputs |got - ref| <= 2^-8 |ref| + 2e-5 max|ref| per element - what accumulating in
   less than float32 would break and small integers cannot see.

Kernel reached by each test id (read off the dispatch - ops.conv2d, conv_bf16_tile.h dispatch_b_t / launch_conv_b, conv_bf16_wgrad.hip
wgrad_bf16_impl, wgrad3.hip, wgrad5.hip - and confirmed by one rocprofv3 --kernel-trace --stats run of this module: every kernel
named below appears in it, with the template arguments the ids say; the table needed no correction).  The 64-channel
tiles and with them conv5_ring_kernel<128|64> need >= 384 workgroups of 64 channels (ids ending in -384wg); below that the
dispatch takes the 32-channel tile, which is what the FAN layer shapes at n = 1 reach (ids tile16buf-tn32-k5-*).

  conv_fwd_packed_bf16_kernel        fwd[packed-*], pool[packed-*]     conv3_rows_c4_kernel       fwd[rows_c4-on]
  conv3_rows_kernel                  fwd[rows-*-on], dgrad[rows-*-on], and_pool[rows-*], rows_d2s
  conv_fwd_bf16_kernel 16x16 TN32    fwd[tile16-tn32-*], dgrad[tile16-*], epilogues[tile16-*]       TN64: fwd / pool[tile16-tn64-*]
  ... buffer loads (bf16 in)         fwd / dgrad / pool / dgrad_unpool[tile16buf-tn32-*], fwd[tile16buf-tn64-*], epilogues[tile16buf-*]
  conv_fwd_bf16_kernel 8x8 x 4       fwd[tile8x4-*] (TN64: tile8x4-tn64-*, tile8x4buf-tn64-*)       32x16: fwd[tile32x16-*]
  conv_fwd_bf16_kernel 1x1 CK16/CK64 fwd[k1-*]                         stride 2: fwd[stride2-*], epilogues[stride2-*]; 2x2: convt2x2
  conv3_dma_kernel pixel-major       fwd / dgrad[dma-*] (TN64: dma-tn64-*), and_pool[dma-*], unpool_out[dma-*]
  conv3_dma_kernel plane (NB = 4)    fwd[dma4-*] (TN64: dma4-tn64-*), dgrad[dma4-*], unpool_out[dma4-*]
  conv5_ring_kernel<128>             fwd / pool / dgrad[ring128-*], dgrad_unpool[ring128-*-dense] (un-pooling input)
  conv5_ring_kernel<64>              fwd / pool / dgrad[ring64-*], dgrad_unpool[ring64-*-dense]
  conv5_ring_kernel<32>              fwd / dgrad[ring32-*], dgrad_unpool[ring32-*-dense]
  conv_dgrad_fewin_bf16_kernel       dgrad[fewin-*], front_end_conv1   conv5_dgrad_sparse_kernel<2>   dgrad_unpool[*-sparse]
  conv_wgrad_bf16_kernel             wgrad[generic-* | narrow-* | pair8-* | k1-* | s2-*], convt2x2 (2x2 / stride 2)
  conv_wgrad_packed_bf16_kernel      wgrad[packed-*], front_end_conv1  conv3_wgrad_alltaps_kernel wgrad[alltaps3-*] (64-wide blocks: alltaps3-nb2-*)
  conv5_wgrad_sparse8_kernel<16>     wgrad_unpool[*-sparse8] at h % 16 == 0        conv5_wgrad_sparse_kernel<16>  wgrad_unpool[*-sparse4]
  conv5_wgrad_alltaps_kernel         wgrad_unpool[*-alltaps] (16-row form), and the h = 8 / h = 24 shapes in every form (8-row form)
  conv_wgrad_c3k5_mfma_kernel        wgrad[c3k5*], front_end_cconv3
  cconv_kernel / cdgrad_border_kernel / conv5c3_mfma_kernel            front_end_cconv3
  conv1_pool_fwd_kernel / conv1_wgrad_pooled_kernel / conv1_dgrad_pooled_kernel   front_end_conv1
  conv_fwd_kernel / conv_fwd_packed_kernel / conv_fewout_kernel (conv_mfma.hip, conv_small.hip)   parity_fwd / parity_dgrad[f32-*]
  conv_wgrad_kernel / conv_wgrad_packed_kernel / conv_wgrad_tiny_kernel / conv_wgrad_c3k5_kernel  parity_wgrad[f32-*]

Not reached here: every kernel behind a switch that csrc/ reads ONCE per process - it cannot be toggled inside one pytest process.
tests/test_gpu_conv_switches.py runs them in child processes (the BUF = false fallbacks of the buffer-load / LDS-DMA / ring routes,
conv5_dgrad_sparse16_kernel, conv5_dgrad_sparse_kernel<4>, the 8-wave ring, the 3x3 ring, the pixel-major NB = 4 DMA tile, the
ticket finish of the weight gradients, ...); its header lists what remains unreached even there, with the reasons (the
NIMG_CONV3_VARIANTS block: compiled out; the ablation switches: not the layer by design).
"""
import time

import numpy as np
import pytest
import torch

from oracle import tfops as T

from util import (assert_exact, assert_exact_conditions, bf16_rne, first_max_pool, lrelu_f32, mask_f32, small_ints, ternary,
                  to64, unpool)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PAD_NAMES = {1: 'SYMMETRIC', 2: 'REFLECT'}
_T0 = [None]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    _T0[0] = time.monotonic()
    yield torch.device('cuda', 0)
    print('exact: module wall time {:.1f} s'.format(time.monotonic() - _T0[0]))        # (shown with pytest -s)


def dv(a, dev, bf=False):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, dtype=np.float32, order='C')).to(dev).contiguous()          # (np.array: always a copy)
    return t.to(BF) if bf else t


def host(t):
    return t.float().cpu().numpy()


def gen(stores_bf16):
    return ternary if stores_bf16 else small_ints


def P(id_, **kw):
    kw['name'] = id_
    return pytest.param(kw, id=id_)


def conv_ref(x, wt, b, stride=1, padding='SAME', pad_mode=0):
    """(float64 oracle, the same convolution of the absolute operands) as numpy arrays."""
    def one(x_, w_, b_):
        xt = to64(x_)
        pd = padding
        if pad_mode:
            xt, pd = T.pad2d(xt, (w_.shape[0] - 1) // 2, PAD_NAMES[pad_mode]), 'VALID'
        return T.conv2d(xt, to64(w_), None if b_ is None else to64(b_), stride, pd).numpy()
    return one(x, wt, b), one(np.abs(x), np.abs(wt), None if b is None else np.abs(b))


def flipped(wt):
    """(k,k,cin,cout) -> the kernel of the input-gradient correlation (k,k,cout,cin), spatially flipped."""
    return np.ascontiguousarray(wt[::-1, ::-1].transpose(0, 1, 3, 2))


def finish(ref, act, stores_bf16):
    """What a kernel must store: the exact value, LeakyReLU as one float32 multiply, one rounding where the output is bf16."""
    want = ref if act is None else lrelu_f32(ref)
    return bf16_rne(want) if (stores_bf16 and act is not None) else np.asarray(want, np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# 1. exact-integer parity: forward
#    shape = (n, h, w, c1, c2, cout, k, stride); xb: x stored as bf16; ob: output storages to run (False float32 / True bf16)
FWD = [
    P('packed-k5c3-symmetric', shape=(2, 40, 72, 3, 0, 32, 5, 1), ob=(False, True), pad_mode=1),
    P('packed-k3c4-reflect', shape=(2, 24, 24, 4, 0, 64, 3, 1), ob=(False, True), pad_mode=2),
    P('packed-k5c4-zero', shape=(1, 18, 34, 4, 0, 24, 5, 1), ob=(False, True)),
    P('rows_c4-on', shape=(2, 20, 128, 4, 0, 32, 3, 1), ob=(True,), rows=True),
    P('packed-k3c4-rows-off', shape=(2, 20, 128, 4, 0, 32, 3, 1), ob=(True,), rows=False),
    P('rows-32-h4-on', shape=(2, 4, 128, 32, 0, 32, 3, 1), xb=True, ob=(True, False), rows=True),
    P('rows-64-h20-on', shape=(2, 20, 128, 64, 0, 32, 3, 1), xb=True, ob=(True, False), rows=True),
    P('rows-32+32-h128-on', shape=(1, 128, 128, 32, 32, 32, 3, 1), xb=True, ob=(True, False), rows=True),
    P('rows-32+32-h20-on', shape=(3, 20, 128, 32, 32, 32, 3, 1), xb=True, ob=(True,), rows=True),
    P('dma-32-h4-rows-off', shape=(2, 4, 128, 32, 0, 32, 3, 1), xb=True, ob=(True, False), rows=False),
    P('tile16buf-64-h20-rows-off', shape=(2, 20, 128, 64, 0, 32, 3, 1), xb=True, ob=(True, False), rows=False),
    P('dma-32+32-h128-rows-off', shape=(1, 128, 128, 32, 32, 32, 3, 1), xb=True, ob=(True,), rows=False),
    P('tile16-tn32-c8', shape=(2, 20, 24, 8, 0, 24, 3, 1), ob=(False, True)),
    P('tile16-tn32-c12', shape=(2, 16, 24, 12, 0, 32, 3, 1), ob=(False,)),
    P('tile16-tn32-c48', shape=(3, 16, 16, 48, 0, 96, 3, 1), ob=(False, True)),
    P('tile16-tn32-k5-c16-ragged', shape=(1, 37, 19, 16, 0, 72, 5, 1), ob=(False,)),
    P('tile16-tn64-k3-f32in-384wg', shape=(6, 128, 128, 8, 0, 64, 3, 1), ob=(False,)),
    P('tile16-valid-k3', shape=(2, 20, 24, 8, 0, 24, 3, 1), ob=(False,), padding='VALID'),
    P('tile16-valid-k5-bf16in', shape=(2, 21, 37, 16, 0, 32, 5, 1), xb=True, ob=(False, True), padding='VALID'),
    P('tile16-two-inputs-f32in', shape=(2, 16, 16, 16, 16, 32, 3, 1), ob=(False,)),
    P('tile16buf-k3-32to64-1600px', shape=(2, 40, 40, 32, 0, 64, 3, 1), xb=True, ob=(False, True)),
    P('tile8x4-k3-64to128', shape=(5, 8, 8, 64, 0, 128, 3, 1), ob=(False, True)),
    P('tile8x4-k5-8to24', shape=(6, 8, 8, 8, 0, 24, 5, 1), ob=(False,)),
    P('tile8x4-tn64-16to512-384wg', shape=(190, 8, 8, 16, 0, 512, 3, 1), ob=(False,)),
    P('tile8x4-k3-5x7-16to40', shape=(7, 5, 7, 16, 0, 40, 3, 1), ob=(False,)),
    P('tile32x16-k5-8to32', shape=(16, 256, 256, 8, 0, 32, 5, 1), ob=(False,)),
    P('k1-ck64-64to64', shape=(3, 16, 16, 64, 0, 64, 1, 1), ob=(False, True)),
    P('k1-ck16-48to32', shape=(3, 16, 16, 48, 0, 32, 1, 1), ob=(False,)),
    P('k1-ck64-64+64', shape=(3, 16, 16, 64, 64, 64, 1, 1), ob=(False,)),
    P('k1-ck64-bf16in', shape=(3, 16, 16, 64, 0, 64, 1, 1), xb=True, ob=(True,)),
    P('stride2-k5-64to128', shape=(2, 32, 32, 64, 0, 128, 5, 2), ob=(False,)),
    P('stride2-k5-16to32-odd', shape=(2, 17, 23, 16, 0, 32, 5, 2), ob=(False,)),
    P('dma-128+128to128', shape=(3, 32, 32, 128, 128, 128, 3, 1), xb=True, ob=(True, False)),
    P('dma-256to256', shape=(5, 16, 16, 256, 0, 256, 3, 1), xb=True, ob=(True, False)),
    P('dma-16to24-ragged', shape=(2, 24, 20, 16, 0, 24, 3, 1), xb=True, ob=(True, False)),
    P('dma4-512to512', shape=(5, 8, 8, 512, 0, 512, 3, 1), xb=True, ob=(True, False)),
    P('dma4-256+256to256', shape=(5, 8, 8, 256, 256, 256, 3, 1), xb=True, ob=(True,)),
    P('dma4-6x8-64to36', shape=(3, 6, 8, 64, 0, 36, 3, 1), xb=True, ob=(True, False)),
    # (below 384 workgroups of 64 channels the dispatch takes the 32-channel tile, not the ring: the FAN shapes at n = 1)
    P('tile16buf-tn32-k5-fan2-32to64-128px', shape=(1, 128, 128, 32, 0, 64, 5, 1), xb=True, ob=(False, True)),
    P('tile16buf-tn32-k5-fan3-64to128-64px', shape=(1, 64, 64, 64, 0, 128, 5, 1), xb=True, ob=(False, True)),
    P('tile16buf-tn32-k5-fan4-128to256-32px', shape=(1, 32, 32, 128, 0, 256, 5, 1), xb=True, ob=(False, True)),
    P('tile16buf-tn32-k5-64to64-ragged', shape=(2, 48, 40, 64, 0, 64, 5, 1), xb=True, ob=(False, True)),
    P('ring64-fan2-32to64-128px-384wg', shape=(6, 128, 128, 32, 0, 64, 5, 1), xb=True, ob=(False, True)),
    P('ring128-fan3-64to128-64px-384wg', shape=(12, 64, 64, 64, 0, 128, 5, 1), xb=True, ob=(False, True)),
    P('ring128-fan4-128to256-32px-384wg', shape=(24, 32, 32, 128, 0, 256, 5, 1), xb=True, ob=(False, True)),
    P('ring64-64to192-ragged-405wg', shape=(15, 48, 40, 64, 0, 192, 5, 1), xb=True, ob=(False, True)),
    P('ring128-24x40-32to512-384wg', shape=(8, 24, 40, 32, 0, 512, 5, 1), xb=True, ob=(False,)),
    P('tile16buf-tn64-k3-16to64-384wg', shape=(6, 128, 128, 16, 0, 64, 3, 1), xb=True, ob=(False, True)),
    P('dma-tn64-16+16to256-384wg', shape=(24, 32, 32, 16, 16, 256, 3, 1), xb=True, ob=(True, False)),
    P('dma-tn64-32to128-ragged-384wg', shape=(48, 24, 20, 32, 0, 128, 3, 1), xb=True, ob=(True,)),
    P('dma4-tn64-16to512-384wg', shape=(190, 8, 8, 16, 0, 512, 3, 1), xb=True, ob=(True, False)),
    P('tile8x4-tn64-bf16in-8to512-384wg', shape=(190, 8, 8, 8, 0, 512, 3, 1), xb=True, ob=(True,)),
    P('tile8x4buf-tn64-k5-16to512-384wg', shape=(190, 8, 8, 16, 0, 512, 5, 1), xb=True, ob=(False,)),
    P('ring32-64to32-ragged', shape=(2, 40, 72, 64, 0, 32, 5, 1), xb=True, ob=(False, True)),
    P('tile16buf-k5-24px-16to64', shape=(2, 24, 24, 16, 0, 64, 5, 1), xb=True, ob=(False,)),
]


def run_fwd(dev, case, monkeypatch, mode):
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout, k, s = case['shape']
    if 'rows' in case:
        monkeypatch.setattr(ops, 'ROWS_CONV', case['rows'])
    ops.set_compute(mode)
    pad_mode, padding, xb = case.get('pad_mode', 0), case.get('padding', 'SAME'), case.get('xb', False)
    for ob in case['ob']:
        G = gen(ob)
        x, wt, b = G((n, h, w, c1 + c2), 1), G((k, k, c1 + c2, cout), 2), G((cout,), 3)
        ref, absum = conv_ref(x, wt, b, s, padding, pad_mode)
        what = '{} {} out {}'.format(mode, case['shape'], 'bf16' if ob else 'f32')
        assert_exact_conditions(absum, ref, ob, what=what)
        x1 = dv(x[..., :c1], dev, xb)
        x2 = dv(x[..., c1:], dev, xb) if c2 else None
        if 'rows' in case and case['rows'] and c1 > 4:
            o = torch.empty((n, h, w, cout), dtype=BF if ob else torch.float32, device=dev)
            assert ops.rows_conv_ok(x1, x2, k, s, cout, (h, w), (1, 1), 0, o, None, None, None)
        for act in (None, 'leaky_relu'):
            out = ops.conv2d(x1, dv(wt, dev), dv(b, dev), x2=x2, stride=s, padding=padding, act=act, pad_mode=pad_mode,
                             out_bf16=ob)
            assert out.dtype == (BF if ob else torch.float32)
            assert_exact(host(out), finish(ref, act, ob), '{} act {}'.format(what, act))


@pytest.mark.parametrize('case', FWD)
def test_fwd_exact(dev, case, monkeypatch):
    run_fwd(dev, case, monkeypatch, 'bf16')


# ----------------------------------------------------------------------------------------------------------------------
# input gradients: shape = (n, h, w, cin, cout, k): dz (n,h,w,cout), kernel (k,k,cin,cout), result (n,h,w,cin)
DGRAD = [
    P('tile16-k3-8from24', shape=(2, 20, 24, 8, 24, 3), ob=(False,), mask='f32'),
    P('tile16-k5-40from72', shape=(1, 37, 19, 40, 72, 5), ob=(False,)),
    P('tile16-k3-two-outputs', shape=(2, 16, 16, 32, 32, 3), ob=(False,), split=True),
    P('rows-32from32-mask-on', shape=(2, 20, 128, 32, 32, 3), zb=True, ob=(True, False), mask='bf16', rows=True),
    P('rows-64from32-two-outputs-on', shape=(2, 20, 128, 64, 32, 3), zb=True, ob=(True,), split=True, rows=True),
    P('rows-64from32-two-outputs-h4-on', shape=(3, 4, 128, 64, 32, 3), zb=True, ob=(True,), split=True, rows=True),
    P('tile-32from32-mask-rows-off', shape=(2, 20, 128, 32, 32, 3), zb=True, ob=(True, False), mask='bf16', rows=False),
    P('tile-64from32-two-outputs-rows-off', shape=(2, 20, 128, 64, 32, 3), zb=True, ob=(True,), split=True, rows=False),
    P('ring32-32from64-ragged', shape=(2, 40, 72, 32, 64, 5), zb=True, ob=(False, True)),
    P('ring32-32from64-mask', shape=(2, 40, 72, 32, 64, 5), zb=True, ob=(True,), mask='bf16'),
    P('tile16buf-tn32-k5-64from128-mask', shape=(1, 64, 64, 64, 128, 5), zb=True, ob=(True, False), mask='bf16'),
    P('tile16buf-tn32-k5-128from256-mask', shape=(1, 32, 32, 128, 256, 5), zb=True, ob=(True,), mask='bf16'),
    P('ring64-64from32-mask-384wg', shape=(6, 128, 128, 64, 32, 5), zb=True, ob=(True, False), mask='bf16'),
    P('ring128-128from64-mask-384wg', shape=(12, 64, 64, 128, 64, 5), zb=True, ob=(True, False), mask='bf16'),
    P('dma-tn64-256from32-mask-384wg', shape=(24, 32, 32, 256, 32, 3), zb=True, ob=(True,), mask='bf16'),
    P('dma-256from256-mask', shape=(5, 16, 16, 256, 256, 3), zb=True, ob=(True,), mask='bf16'),
    P('dma4-512from512', shape=(5, 8, 8, 512, 512, 3), zb=True, ob=(True,)),
    P('fewin-3from32-32x80', shape=(3, 32, 80, 3, 32, 5), ob=(False,)),
    P('fewin-3from32-20x36', shape=(2, 20, 36, 3, 32, 5), ob=(False,)),
]


def run_dgrad(dev, case, monkeypatch, mode):
    from neural_imaging_amd import ops
    n, h, w, cin, cout, k = case['shape']
    if 'rows' in case:
        monkeypatch.setattr(ops, 'ROWS_CONV', case['rows'])
    ops.set_compute(mode)
    zb, mask_kind, split = case.get('zb', False), case.get('mask'), case.get('split', False)
    for ob in case['ob']:
        G = gen(ob)
        dz, wt = G((n, h, w, cout), 4), G((k, k, cin, cout), 5)
        ref, absum = conv_ref(dz, flipped(wt), None)
        what = 'dgrad {} {} out {}'.format(mode, case['shape'], 'bf16' if ob else 'f32')
        assert_exact_conditions(absum, ref, ob, what=what)
        dzd, wd = dv(dz, dev, zb), dv(wt, dev)
        plain = ops.conv2d_dgrad(dzd, wd, (h, w), out_bf16=ob) if not split else None
        if split:
            dt = BF if ob else torch.float32
            o1, o2 = torch.empty((n, h, w, cin // 2), dtype=dt, device=dev), torch.empty((n, h, w, cin // 2), dtype=dt, device=dev)
            ops.conv2d_dgrad(dzd, wd, (h, w), out=o1, out2=o2)
            plain = torch.cat([o1, o2], dim=-1)
        assert plain.dtype == (BF if ob else torch.float32)
        assert_exact(host(plain), ref, what)
        if mask_kind:
            m = small_ints((n, h, w, cin), 6, 1)
            got = ops.conv2d_dgrad(dzd, wd, (h, w), act_mask=dv(m, dev, mask_kind == 'bf16'), out_bf16=ob)
            want = mask_f32(ref, m)
            assert_exact(host(got), bf16_rne(want) if ob else want, what + " x LeakyReLU'")


@pytest.mark.parametrize('case', DGRAD)
def test_dgrad_exact(dev, case, monkeypatch):
    run_dgrad(dev, case, monkeypatch, 'bf16')


# ----------------------------------------------------------------------------------------------------------------------
# weight gradients: shape = (n, h, w, c1, c2, cout, k, stride); xb / zb: operands stored as bf16
WGRAD = [
    P('narrow-k3-8to24', shape=(2, 20, 24, 8, 0, 24, 3, 1)),
    P('generic-k3-48to96-n3', shape=(3, 16, 16, 48, 0, 96, 3, 1)),
    P('generic-k3-two-inputs', shape=(2, 16, 16, 16, 16, 32, 3, 1)),
    P('generic-k3-12to36', shape=(2, 16, 24, 12, 0, 36, 3, 1)),
    P('generic-k5-32to64-n5', shape=(5, 32, 32, 32, 0, 64, 5, 1)),
    P('generic-k5-ragged-40to72', shape=(1, 37, 19, 40, 0, 72, 5, 1)),
    P('generic-k5-bf16-both', shape=(3, 24, 40, 32, 0, 64, 5, 1), xb=True, zb=True),
    P('generic-k3-bf16-x-only', shape=(3, 16, 24, 32, 0, 64, 3, 1), xb=True),
    P('generic-k3-bf16-dz-only', shape=(3, 16, 24, 32, 0, 64, 3, 1), zb=True),
    P('k1-64to64', shape=(3, 16, 16, 64, 0, 64, 1, 1)),
    P('k1-48to32-bf16', shape=(5, 16, 20, 48, 0, 32, 1, 1), xb=True, zb=True),
    P('s2-k5-16to32', shape=(2, 32, 32, 16, 0, 32, 5, 2)),
    P('s2-k5-64to128-n3', shape=(3, 32, 32, 64, 0, 128, 5, 2)),
    P('packed-k5c3', shape=(2, 40, 72, 3, 0, 32, 5, 1)),
    P('packed-k3c4-64out', shape=(2, 24, 24, 4, 0, 64, 3, 1)),
    P('packed-k3c4-rows-shape', shape=(3, 20, 128, 4, 0, 32, 3, 1)),
    P('pair8-64to128-n5', shape=(5, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True),
    P('pair8-512to512-n5', shape=(5, 8, 8, 512, 0, 512, 3, 1), xb=True, zb=True),
    P('alltaps3-32to32-128px', shape=(3, 128, 128, 32, 0, 32, 3, 1), xb=True, zb=True),
    P('alltaps3-32+32to32', shape=(2, 128, 128, 32, 32, 32, 3, 1), xb=True, zb=True),
    P('alltaps3-128+128to128-n5', shape=(5, 32, 32, 128, 128, 128, 3, 1), xb=True, zb=True),
    P('alltaps3-256to256-n7', shape=(7, 16, 16, 256, 0, 256, 3, 1), xb=True, zb=True),
    P('alltaps3-ragged-64to32', shape=(2, 24, 32, 64, 0, 32, 3, 1), xb=True, zb=True),
    P('alltaps3-nb2-32to64-64px', shape=(3, 64, 64, 32, 0, 64, 3, 1), xb=True, zb=True),
    P('alltaps3-nb2-64+64to192', shape=(3, 32, 32, 64, 64, 192, 3, 1), xb=True, zb=True),
    P('c3k5', shape=(2, 24, 64, 3, 0, 3, 5, 1), pad_mode=1, no_db=True),
    P('c3k5-ragged', shape=(1, 37, 128, 3, 0, 3, 5, 1), pad_mode=1, no_db=True),
]


def wgrad_ref(x, dz, k, stride, pad_mode=0):
    def one(x_, dz_):
        wt = torch.zeros((k, k, x_.shape[3], dz_.shape[3]), dtype=torch.float64, requires_grad=True)
        xt = to64(x_)
        if pad_mode:
            z = T.conv2d(T.pad2d(xt, (k - 1) // 2, PAD_NAMES[pad_mode]), wt, None, stride, 'VALID')
        else:
            z = T.conv2d(xt, wt, None, stride, 'SAME')
        assert tuple(z.shape) == tuple(dz_.shape)
        (z * to64(dz_)).sum().backward()
        return wt.grad.numpy()
    return one(x, dz), one(np.abs(x), np.abs(dz))


def run_wgrad(dev, case, mode):
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout, k, s = case['shape']
    ops.set_compute(mode)
    pad_mode, xb, zb = case.get('pad_mode', 0), case.get('xb', False), case.get('zb', False)
    ho, wo = -(-h // s), -(-w // s)
    x, dz = small_ints((n, h, w, c1 + c2), 7), small_ints((n, ho, wo, cout), 8)
    ref, absum = wgrad_ref(x, dz, k, s, pad_mode)
    what = 'wgrad {} {}'.format(mode, case['shape'])
    assert_exact_conditions(absum + 100.0, ref, False, what=what)                  # (+ the integer dw it is accumulated onto)
    assert_exact_conditions(np.abs(dz).sum(axis=(0, 1, 2)), ref, False, what=what + ' (bias)')
    x1, x2, dzd = dv(x[..., :c1], dev, xb), (dv(x[..., c1:], dev, xb) if c2 else None), dv(dz, dev, zb)
    kw = dict(x2=x2, stride=s, pad_mode=pad_mode)
    if pad_mode:
        kw['pads'] = ((k - 1) // 2, (k - 1) // 2)
    dw = torch.full((k, k, c1 + c2, cout), 7.0, device=dev)
    db = None if case.get('no_db') else torch.full((cout,), 7.0, device=dev)
    ops.conv2d_wgrad(x1, dzd, k, dw=dw, db=db, **kw)
    assert_exact(host(dw), ref, what)
    if db is not None:
        assert_exact(host(db), dz.astype(np.float64).sum(axis=(0, 1, 2)), what + ' fused bias gradient')
    dw0 = small_ints((k, k, c1 + c2, cout), 9, 100)
    acc = dv(dw0, dev)
    ops.conv2d_wgrad(x1, dzd, k, dw=acc, accumulate=True, **kw)
    assert_exact(host(acc), ref + dw0, what + ' accumulated onto an integer dw')


@pytest.mark.parametrize('case', WGRAD)
def test_wgrad_exact(dev, case):
    run_wgrad(dev, case, 'bf16')


# ----------------------------------------------------------------------------------------------------------------------
# fused conv + pool (FAN) and its backward from the pooled gradient
POOL = [
    P('tile16buf-tn32-k5-fan2-32to64-128px', shape=(1, 128, 128, 32, 64, 5), xb=True, ob=True),
    P('tile16buf-tn32-k5-fan3-64to128', shape=(1, 64, 64, 64, 128, 5), xb=True, ob=True),
    P('tile16buf-tn32-k5-64to64-ragged', shape=(2, 48, 40, 64, 64, 5), xb=True, ob=True),
    P('ring64-fan2-32to64-128px-384wg', shape=(6, 128, 128, 32, 64, 5), xb=True, ob=True),
    P('ring128-fan3-64to128-64px-384wg', shape=(12, 64, 64, 64, 128, 5), xb=True, ob=True),
    P('ring128-fan4-128to256-32px-384wg', shape=(24, 32, 32, 128, 256, 5), xb=True, ob=True),
    P('ring64-64to192-ragged-405wg', shape=(15, 48, 40, 64, 192, 5), xb=True, ob=True),
    P('ring128-24x40-32to512-f32out-384wg', shape=(8, 24, 40, 32, 512, 5), xb=True, ob=False),
    P('tile16-tn64-f32in-16to64-k5-384wg', shape=(6, 128, 128, 16, 64, 5), ob=False),
    P('tile16-f32in-64to64-k5', shape=(2, 48, 40, 64, 64, 5), ob=False),
    P('tile16-f32in-16to24-k3', shape=(3, 16, 16, 16, 24, 3), ob=False),
    P('tile8x4-6x10-8to256-k5', shape=(3, 6, 10, 8, 256, 5), ob=False),
    P('packed-c3-k5', shape=(3, 32, 48, 3, 32, 5), ob=False),
    P('packed-c4-k3-bf16out', shape=(3, 18, 34, 4, 64, 3), ob=True),
]


@pytest.mark.parametrize('case', POOL)
def test_conv_pool_exact(dev, case):
    """ops.conv2d_pool: pooled values AND every arg-max byte (first maximum in the order (0,0), (0,1), (1,0), (1,1))."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    n, h, w, cin, cout, k = case['shape']
    ob = case['ob']
    G = gen(ob)
    x, wt, b = G((n, h, w, cin), 11), G((k, k, cin, cout), 12), G((cout,), 13)
    ref, absum = conv_ref(x, wt, b)
    assert_exact_conditions(absum, ref, ob, what=str(case['shape']))
    for act in ('leaky_relu', None):
        full = ref if act is None else lrelu_f32(ref).astype(np.float64)
        want, want_idx = first_max_pool(full)
        pooled, idx = ops.conv2d_pool(dv(x, dev, case.get('xb', False)), dv(wt, dev), dv(b, dev), act=act, out_bf16=ob)
        assert_exact(host(pooled), bf16_rne(want) if (ob and act) else want, 'pooled, act {}'.format(act))
        assert (want_idx != first_max_pool(full, last=True)[1]).any(), 'the case has no ties'
        assert_exact(idx.cpu().numpy(), want_idx, 'arg-max bytes, act {}'.format(act))


AND_POOL = [
    P('dma-256to256', shape=(5, 16, 16, 256, 256)), P('dma-16to24-ragged', shape=(2, 24, 20, 16, 24)),
    P('tile16buf-64to64-64px', shape=(2, 64, 64, 64, 64)), P('tile-8to72-10x18', shape=(1, 10, 18, 8, 72)),
    P('rows-32to32', shape=(2, 20, 128, 32, 32), rows=True), P('tile-32to32-rows-off', shape=(2, 20, 128, 32, 32), rows=False),
]


@pytest.mark.parametrize('case', AND_POOL)
def test_conv_and_pool_exact(dev, case, monkeypatch):
    """ops.conv2d_and_pool: the bf16 activation and its max-pool from one epilogue."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    if 'rows' in case:
        monkeypatch.setattr(ops, 'ROWS_CONV', case['rows'])
    n, h, w, cin, cout = case['shape']
    x, wt, b = ternary((n, h, w, cin), 14), ternary((3, 3, cin, cout), 15), ternary((cout,), 16)
    ref, absum = conv_ref(x, wt, b)
    assert_exact_conditions(absum, ref, True, what=str(case['shape']))
    for act in ('leaky_relu', None):
        want = finish(ref, act, True)
        y, pooled = ops.conv2d_and_pool(dv(x, dev, True), dv(wt, dev), dv(b, dev), act=act)
        assert_exact(host(y), want, 'activation, act {}'.format(act))
        assert_exact(host(pooled), first_max_pool(want)[0], 'pooled, act {}'.format(act))


@pytest.mark.parametrize('sparse', [False, True], ids=['dense', 'sparse'])
@pytest.mark.parametrize('shape', [
    pytest.param((2, 32, 32, 32, 64), id='ring32-32from64'), pytest.param((1, 128, 128, 32, 64), id='ring32-32from64-128px'),
    pytest.param((1, 64, 64, 64, 128), id='tile16buf-tn32-64from128'), pytest.param((2, 16, 48, 128, 256), id='tile16buf-tn32-128from256'),
    pytest.param((2, 48, 40, 64, 64), id='tile16buf-tn32-64from64-ragged'),
    pytest.param((6, 128, 128, 64, 64), id='ring64-64from64-128px-384wg'), pytest.param((12, 64, 64, 128, 64), id='ring128-128from64-64px-384wg'),
    pytest.param((15, 48, 40, 192, 64), id='ring64-192from64-ragged-405wg')])
def test_dgrad_unpool_exact(dev, shape, sparse, monkeypatch):
    """ops.conv2d_dgrad_unpool: the 5x5 input gradient read from (pooled gradient, arg-max bytes).  The ids name the kernel of the
    dense form (SPARSE_DGRAD off: un-pooling while staging in the ring / buffer-load tile kernels); the sparse form is
    conv5_dgrad_sparse_kernel<2> of dgrad5s.hip at every shape."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    monkeypatch.setattr(ops, 'SPARSE_DGRAD', sparse)
    n, h, w, cin, cout = shape
    for ob in (False, True):
        G = gen(ob)
        gp, wt = G((n, h // 2, w // 2, cout), 17), G((5, 5, cin, cout), 18)
        idx = np.random.default_rng(19).integers(0, 4, size=gp.shape).astype(np.uint8)
        ref, absum = conv_ref(unpool(gp, idx), flipped(wt), None)
        assert_exact_conditions(absum, ref, ob, what=str(shape))
        gd, idd = dv(gp, dev, True), torch.from_numpy(idx).to(dev)
        assert_exact(host(ops.conv2d_dgrad_unpool(gd, idd, dv(wt, dev), out_bf16=ob)), ref, 'dgrad from the pooled gradient')
        m = small_ints((n, h, w, cin), 20, 1)
        got = ops.conv2d_dgrad_unpool(gd, idd, dv(wt, dev), act_mask=dv(m, dev, True), out_bf16=ob)
        want = mask_f32(ref, m)
        assert_exact(host(got), bf16_rne(want) if ob else want, "dgrad from the pooled gradient x LeakyReLU'")


@pytest.mark.parametrize('form', ['sparse8', 'sparse4', 'alltaps'])
@pytest.mark.parametrize('shape', [(4, 128, 128, 32, 64), (5, 64, 64, 64, 128), (7, 32, 32, 128, 256), (1, 8, 16, 32, 64),
                                   (3, 24, 32, 64, 192)])
def test_wgrad_unpool_exact(dev, shape, form, monkeypatch):
    """ops.conv2d_wgrad_unpool (wgrad5.hip): weight and bias gradient from the pooled gradient.  h % 16 == 0 takes
    conv5_wgrad_sparse8_kernel<16> by default; the two switches the library reads per call select conv5_wgrad_sparse_kernel<16>
    (NIMG_WGRAD5_W4) and the 16-row conv5_wgrad_alltaps_kernel (NIMG_NO_WGRAD5_SPARSE); h = 8 and h = 24 take the 8-row
    conv5_wgrad_alltaps_kernel in every form."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    if form == 'sparse4':
        monkeypatch.setenv('NIMG_WGRAD5_W4', '1')
    elif form == 'alltaps':
        monkeypatch.setenv('NIMG_NO_WGRAD5_SPARSE', '1')
    n, h, w, cin, cout = shape
    x, gp = small_ints((n, h, w, cin), 21), small_ints((n, h // 2, w // 2, cout), 22)
    idx = np.random.default_rng(23).integers(0, 4, size=gp.shape).astype(np.uint8)
    dz = unpool(gp, idx)
    ref, absum = wgrad_ref(x, dz, 5, 1)
    assert_exact_conditions(absum, ref, False, what=str(shape))
    xd, gd, idd = dv(x, dev, True), dv(gp, dev, True), torch.from_numpy(idx).to(dev)
    assert ops.unpool_fold_ok(xd, gd, cin, cout, 5)
    dw, db = torch.full((5, 5, cin, cout), 7.0, device=dev), torch.full((cout,), 7.0, device=dev)
    ops.conv2d_wgrad_unpool(xd, gd, idd, 5, dw, db=db)
    assert_exact(host(dw), ref, 'wgrad from the pooled gradient')
    assert_exact(host(db), dz.astype(np.float64).sum(axis=(0, 1, 2)), 'bias gradient from the pooled gradient')


@pytest.mark.parametrize('with_skip', [True, False], ids=['skip', 'noskip'])
@pytest.mark.parametrize('shape', [
    pytest.param((3, 32, 64, 64, 64), id='tile16buf-32from64-64px'), pytest.param((3, 64, 128, 32, 32), id='dma-64from128-32px'),
    pytest.param((5, 128, 256, 16, 16), id='dma-128from256-16px'), pytest.param((5, 256, 512, 8, 8), id='dma4-256from512-8px'),
    pytest.param((2, 16, 24, 12, 20), id='dma-16from24-ragged'), pytest.param((1, 8, 72, 6, 10), id='tile-8from72-6x10')])
def test_dgrad_unpool_out_exact(dev, shape, with_skip):
    """ops.conv2d_dgrad_unpool_out: 3x3 input gradient (a bf16 value) routed through the 2x2 max-pool to the first maximum of the
    stored activation, + the skip gradient, x LeakyReLU'(activation): shapes of test_input_gradient_written_through_the_max_pool."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    n, cin, cout, h, w = shape
    dz, wt = ternary((n, h, w, cout), 24), ternary((3, 3, cin, cout), 25)
    act = small_ints((n, 2 * h, 2 * w, cin), 26, 2)                       # few distinct values: ties in most windows
    skip = ternary((n, 2 * h, 2 * w, cin), 27, 0.5) if with_skip else None
    ref, absum = conv_ref(dz, flipped(wt), None)
    assert_exact_conditions(absum + 1.0, np.abs(ref) + 1.0, True, what=str(shape))          # + the skip term
    _, idx = first_max_pool(act)
    routed = unpool(ref, idx) + (0.0 if skip is None else skip)
    dzd, wd, ad, sd = dv(dz, dev, True), dv(wt, dev), dv(act, dev, True), dv(skip, dev, True)
    assert ops.conv2d_dgrad_unpool_out_ok(dzd, wd, ad, sd)
    for mask in (False, True):
        want = bf16_rne(mask_f32(routed, act)) if mask else routed
        assert_exact(host(ops.conv2d_dgrad_unpool_out(dzd, wd, ad, skip=sd, apply_mask=mask)), want, 'mask {}'.format(mask))


# ----------------------------------------------------------------------------------------------------------------------
# fused epilogues, stride-2 layers over the space-to-depth image, Conv2DTranspose
def _epi_k3(dev, ops, xb, route):
    """3x3, 32 -> 32 channels at 24 x 40 (16x16 tiles, float32 or bf16-stored input): residual / bf16 copy epilogues."""
    n, h, w, c = 2, 24, 40, 32
    x, r, wt, b = small_ints((n, h, w, c), 31), small_ints((n, h, w, c), 32), small_ints((3, 3, c, c), 33), small_ints((c,), 34)
    ref, absum = conv_ref(x, wt, b)
    assert_exact_conditions(absum + 3.0, ref + r, False)
    xd, wd, bd, rd = dv(x, dev, xb), dv(wt, dev), dv(b, dev), dv(r, dev)
    if route == 'residual':
        assert_exact(host(ops.conv2d(xd, wd, bd, residual=rd)), ref + r, 'residual')
        y, cp = ops.conv2d(xd, wd, bd, residual=rd, bf16_copy=True)
        assert_exact(host(y), ref + r, 'residual + copy')
        assert_exact(host(cp), bf16_rne(ref + r), 'the bf16 copy')
    elif route == 'bf16_copy':
        y, cp = ops.conv2d(xd, wd, bd, act='leaky_relu', bf16_copy=True)
        assert_exact(host(y), lrelu_f32(ref), 'lrelu + copy')
        assert_exact(host(cp), bf16_rne(lrelu_f32(ref)), 'the bf16 copy')
    elif route == 'copy_lrelu':
        y, cp = ops.conv2d(xd, wd, bd, bf16_copy=True, copy_lrelu=True)
        assert_exact(host(y), ref, 'plain + LeakyReLU copy')
        assert_exact(host(cp), bf16_rne(lrelu_f32(ref)), 'the LeakyReLU copy')
    else:
        dref, dabs = conv_ref(x, flipped(wt), None)
        assert_exact_conditions(dabs + 3.0, dref + r, False)
        assert_exact(host(ops.conv2d_dgrad(xd, wd, (h, w), residual=rd)), dref + r, 'dgrad + residual')


def _epi_k5(dev, ops, route):
    """5x5 with a bf16 copy: stays on the generic buffer-load tile at a ring shape; stride 2 with the LeakyReLU copy."""
    x5, w5, b5 = ternary((2, 48, 40, 64), 35), ternary((5, 5, 64, 64), 36), ternary((64,), 37)
    if route == 'bf16_copy':
        ref5, abs5 = conv_ref(x5, w5, b5)
        assert_exact_conditions(abs5, ref5, True)
        y, cp = ops.conv2d(dv(x5, dev, True), dv(w5, dev), dv(b5, dev), act='leaky_relu', bf16_copy=True)
        assert_exact(host(y), lrelu_f32(ref5), 'k5 + copy')
        assert_exact(host(cp), bf16_rne(lrelu_f32(ref5)), 'k5: the bf16 copy')
    else:
        refs, abss = conv_ref(x5, w5, None, 2)
        assert_exact_conditions(abss, refs, True)
        y, cp = ops.conv2d(dv(x5, dev), dv(w5, dev), None, stride=2, bf16_copy=True, copy_lrelu=True)
        assert_exact(host(y), refs, 'stride 2 + copy')
        assert_exact(host(cp), bf16_rne(lrelu_f32(refs)), 'stride 2: the LeakyReLU copy')


def _epi_d2s(dev, ops, ob, mask):
    """depth_to_space written by the 3x3 epilogue: plain (both activations), and x LeakyReLU' of a mask given in the output's
    layout (float32) or in the convolution's own layout, i.e. as the bf16 space-to-depth image of the activation (mask_conv_layout)."""
    n, h, w, cin, cout = 2, 12, 20, 32, 64
    G = gen(ob)
    x, wt, b = G((n, h, w, cin), 38), G((3, 3, cin, cout), 39), G((cout,), 40)
    ref, absum = conv_ref(x, wt, b)
    assert_exact_conditions(absum, ref, ob)
    d2s = lambda a: T.depth_to_space(to64(a), 2).numpy()
    if mask is None:
        for act in (None, 'leaky_relu'):
            got = ops.conv2d(dv(x, dev), dv(wt, dev), dv(b, dev), act=act, d2s_out=True, out_bf16=ob)
            assert_exact(host(got), d2s(finish(ref, act, ob)), 'd2s_out act {} bf16 {}'.format(act, ob))
        return
    m = small_ints((n, 2 * h, 2 * w, cout // 4), 49, 1)                  # the mask where the result lands
    want = mask_f32(d2s(ref), m)
    want = bf16_rne(want) if ob else want
    for xb in (False, True):
        if mask == 'output-layout':
            got = ops.conv2d(dv(x, dev, xb), dv(wt, dev), dv(b, dev), d2s_out=True, out_bf16=ob, act_mask=dv(m, dev))
        else:
            ms = dv(T.space_to_depth(to64(m), 2).numpy(), dev, True)
            assert tuple(ms.shape) == (n, h, w, cout)
            got = ops.conv2d(dv(x, dev, xb), dv(wt, dev), dv(b, dev), d2s_out=True, out_bf16=ob, act_mask=ms, mask_conv_layout=True)
        assert got.dtype == (BF if ob else torch.float32)
        assert_exact(host(got), want, 'd2s_out x mask ({}), x bf16 {}, out bf16 {}'.format(mask, xb, ob))


def _epi_s2d(dev, ops, ob, cg):
    """space_to_depth of an input gradient written by the 3x3 epilogue (12 channels: the codec's last layer), plain and masked."""
    n, h, w = 2, 12, 20
    G = gen(ob)
    gz, wz = G((n, h, w, cg), 41 + cg), G((3, 3, 64, cg), 42 + cg)
    dref, dabs = conv_ref(gz, flipped(wz), None)
    assert_exact_conditions(dabs, dref, ob)
    m = small_ints((n, h, w, 64), 43, 1)
    got = ops.conv2d_dgrad(dv(gz, dev), dv(wz, dev), (h, w), s2d_out=True, out_bf16=ob)
    assert_exact(host(got), T.space_to_depth(to64(dref), 2).numpy(), 's2d_out cg {} bf16 {}'.format(cg, ob))
    got = ops.conv2d_dgrad(dv(gz, dev), dv(wz, dev), (h, w), s2d_out=True, out_bf16=ob, act_mask=dv(m, dev))
    want = mask_f32(dref, m)
    assert_exact(host(got), T.space_to_depth(to64(bf16_rne(want) if ob else want), 2).numpy(), 's2d_out + mask cg {}'.format(cg))


EPILOGUES = [pytest.param(lambda d, o, xb=xb, r=r: _epi_k3(d, o, xb, r), id='tile16{}-k3-{}'.format('-bf16in' if xb else '', r))
             for xb in (False, True) for r in ('residual', 'bf16_copy', 'copy_lrelu', 'dgrad-residual')] + [
    pytest.param(lambda d, o: _epi_k5(d, o, 'bf16_copy'), id='tile16buf-tn32-k5-bf16_copy-at-a-ring-shape'),
    pytest.param(lambda d, o: _epi_k5(d, o, 'copy_lrelu'), id='stride2-k5-copy_lrelu')] + [
    pytest.param(lambda d, o, ob=ob, mk=mk: _epi_d2s(d, o, ob, mk), id='tile16-k3-d2s_out-{}-{}'.format(mk or 'plain', 'bf16out' if ob else 'f32out'))
    for ob in (False, True) for mk in (None, 'output-layout', 'mask_conv_layout')] + [
    pytest.param(lambda d, o, ob=ob, cg=cg: _epi_s2d(d, o, ob, cg), id='tile16-k3-s2d_out-{}ch-{}'.format(cg, 'bf16out' if ob else 'f32out'))
    for ob in (False, True) for cg in (12, 16)]


@pytest.mark.parametrize('run', EPILOGUES)
def test_epilogues_exact(dev, run):
    """residual, bf16_copy, copy_lrelu, d2s_out (with a mask in either layout), s2d_out (12 and 16 channels) - each against the
    oracle, not against the plain call (two-tensor outputs, out2: test_dgrad_exact[*two-outputs*])."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    run(dev, ops)


@pytest.mark.parametrize('shape', [(2, 24, 40, 64, 32), (2, 32, 48, 3, 64), (1, 16, 16, 8, 16)])
def test_stride2_as_space_to_depth_exact(dev, shape):
    """A 5x5 stride-2 SAME layer as a 3x3 layer over the bf16 space-to-depth image (ops.s2d2_affine / s2d_conv_weights), its
    weight gradient through s2d_conv_weights_bwd and its input gradient (ops.conv2d_dgrad_strided2, depth-to-space epilogue)."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    n, h, w, cin, cout = shape
    x, wt, b = small_ints((n, h, w, cin), 44), small_ints((5, 5, cin, cout), 45), small_ints((cout,), 46)
    ref, absum = conv_ref(x, wt, b, 2)
    assert_exact_conditions(absum, ref, False, what=str(shape))
    xs = ops.s2d2_affine(dv(x, dev), 1.0, 0.0)
    w3 = ops.s2d_conv_weights(dv(wt, dev))
    assert xs.dtype == BF and xs.shape[3] == w3.shape[2]
    assert_exact(host(ops.conv2d(xs, w3, dv(b, dev))), ref, 'forward over the space-to-depth image')
    dz = small_ints(ref.shape, 47)
    wref, wabs = wgrad_ref(x, dz, 5, 2)
    assert_exact_conditions(wabs, wref, False)
    dw3 = ops.conv2d_wgrad(xs, dv(dz, dev), 3)
    dw5 = ops.s2d_conv_weights_bwd(dw3, torch.zeros((5, 5, cin, cout), device=dev))
    assert_exact(host(dw5), wref, 'weight gradient over the space-to-depth image')
    xt = to64(x).requires_grad_(True)
    (T.conv2d(xt, to64(wt), None, 2, 'SAME') * to64(dz)).sum().backward()
    xa = to64(np.abs(x)).requires_grad_(True)
    (T.conv2d(xa, to64(np.abs(wt)), None, 2, 'SAME') * to64(np.abs(dz))).sum().backward()
    assert_exact_conditions(xa.grad.numpy(), xt.grad.numpy(), False)
    assert_exact(host(ops.conv2d_dgrad_strided2(dv(dz, dev), dv(wt, dev), (h, w))), xt.grad.numpy(), 'input gradient')
    if cin % 4 == 0:
        m = small_ints((n, h, w, cin), 48, 1)
        got = ops.conv2d_dgrad_strided2(dv(dz, dev), dv(wt, dev), (h, w), act_mask=dv(m, dev))
        assert_exact(host(got), mask_f32(xt.grad.numpy(), m), "input gradient x LeakyReLU'")


@pytest.mark.parametrize('xb', [False, True], ids=['f32', 'bf16stored'])
@pytest.mark.parametrize('shape', [(5, 8, 8, 512, 256), (3, 16, 20, 24, 40), (2, 64, 64, 64, 32), (2, 8, 12, 64, 32)])
def test_convt2x2_exact(dev, shape, xb):
    """Conv2DTranspose(2, stride 2): forward, input gradient (the 2x2 / stride-2 tile kernel) and weight gradient."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    n, h, w, cin, cout = shape
    for ob in ((False, True) if xb else (False,)):
        G = gen(ob)
        x, wt, b = G((n, h, w, cin), 51), G((2, 2, cout, cin), 52), G((cout,), 53)
        ref = T.conv2d_transpose_2x2(to64(x), to64(wt), to64(b)).numpy()
        absum = T.conv2d_transpose_2x2(to64(np.abs(x)), to64(np.abs(wt)), to64(np.abs(b))).numpy()
        assert_exact_conditions(absum, ref, ob, what=str(shape))
        assert_exact(host(ops.convt2x2(dv(x, dev, xb), dv(wt, dev), dv(b, dev), out_bf16=ob)), ref, 'convT forward')
        dy = G((n, 2 * h, 2 * w, cout), 54)
        xt, wtt = to64(x).requires_grad_(True), to64(wt).requires_grad_(True)
        (T.conv2d_transpose_2x2(xt, wtt, None) * to64(dy)).sum().backward()
        xa, wa = to64(np.abs(x)).requires_grad_(True), to64(np.abs(wt)).requires_grad_(True)
        (T.conv2d_transpose_2x2(xa, wa, None) * to64(np.abs(dy))).sum().backward()
        assert_exact_conditions(xa.grad.numpy(), xt.grad.numpy(), ob)
        assert_exact_conditions(wa.grad.numpy(), wtt.grad.numpy(), False)
        m = small_ints((n, h, w, cin), 55, 1)
        dyd = dv(dy, dev, xb)
        assert_exact(host(ops.convt2x2_dgrad(dyd, dv(wt, dev), out_bf16=ob)), xt.grad.numpy(), 'convT input gradient')
        got = ops.convt2x2_dgrad(dyd, dv(wt, dev), act_mask=dv(m, dev, xb), out_bf16=ob)
        want = mask_f32(xt.grad.numpy(), m)
        assert_exact(host(got), bf16_rne(want) if ob else want, "convT input gradient x LeakyReLU'")
        assert_exact(host(ops.convt2x2_wgrad(dv(x, dev, xb), dyd)), wtt.grad.numpy(), 'convT weight gradient')


def test_rows_d2s_exact(dev, monkeypatch):
    """ops.conv3_rows_d2s (the UNet's last layer): clip(depth_to_space(conv), 0, 1); the 2^-6 scale on the kernel keeps every value
    exact and puts results inside and outside [0, 1]."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    sc = 2.0 ** -6
    for n, h in ((2, 4), (2, 20), (1, 128)):
        x, wt, b = small_ints((n, h, 128, 32), 56), small_ints((3, 3, 32, 12), 57) * np.float32(sc), small_ints((12,), 58) * np.float32(sc)
        ref, absum = conv_ref(x, wt, b)
        assert_exact_conditions(absum, ref, False, scale=sc)
        want = np.clip(T.depth_to_space(to64(ref), 2).numpy(), 0.0, 1.0)
        assert 0.1 < (want == 0).mean() < 0.9 and (want == 1).mean() > 0.01 and ((want > 0) & (want < 1)).mean() > 0.05
        xd = dv(x, dev, True)
        for on in (True, False):
            monkeypatch.setattr(ops, 'ROWS_CONV', on)
            got = ops.conv3_rows_d2s(xd, dv(wt, dev), dv(b, dev)) if on else \
                ops.d2s_clip(ops.conv2d(xd, dv(wt, dev), dv(b, dev)), 1.0, 0.0, True)
            assert_exact(host(got), want, 'rows d2s {} h {}'.format(on, h))


# ----------------------------------------------------------------------------------------------------------------------
# FAN front end
@pytest.mark.parametrize('shape', [(2, 24, 64), (1, 37, 128), (1, 5, 192), (2, 256, 256)])
def test_front_end_cconv3_exact(dev, shape):
    """cconv_kernel (+ its bf16 pixel), the input gradient as a stencil (parity mode) and on the matrix core (conv5c3_mfma_kernel,
    widths that are multiples of 64) with the SYMMETRIC-pad border fold, and the 5x5x3x3 weight gradient (c3k5)."""
    from neural_imaging_amd import ops
    n, h, w = shape
    x, k = ternary((n, h, w, 3), 61, 0.5), small_ints((5, 5, 3, 3), 62)
    ref, absum = conv_ref(x, k, None, pad_mode=1)
    assert_exact_conditions(absum, ref, True, what=str(shape))
    y, c4 = ops.cconv3(dv(x, dev), dv(k, dev), pad_mode=1, want_c4=True)
    assert_exact(host(y), ref, 'cconv3')
    assert_exact(host(c4), np.concatenate([ref, np.ones((n, h, w, 1))], axis=-1), 'cconv3: the bf16 {y, 1} pixel')
    dy = small_ints((n, h, w, 3), 63)
    xt = to64(x).requires_grad_(True)
    (T.conv2d(T.pad2d(xt, 2, 'SYMMETRIC'), to64(k), None, 1, 'VALID') * to64(dy)).sum().backward()
    for mode in ('f32', 'bf16'):
        ops.set_compute(mode)
        assert_exact(host(ops.cconv3_dgrad(dv(dy, dev), dv(k, dev))), xt.grad.numpy(), 'cconv3 input gradient, ' + mode)
        run_wgrad(dev, dict(shape=(n, h, w, 3, 0, 3, 5, 1), pad_mode=1, no_db=True), mode)


@pytest.mark.parametrize('shape', [(2, 24, 64), (1, 36, 128), (1, 6, 192), (2, 256, 256)])
def test_front_end_conv1_exact(dev, shape):
    """conv1_pool_fwd_kernel (values and EVERY 2-bit arg-max code), conv1_wgrad_pooled_kernel, conv1_dgrad_pooled_kernel."""
    from neural_imaging_amd import ops
    from test_gpu_ops import pack_argmax2, unpack_argmax2
    ops.set_compute('bf16')
    n, h, w = shape
    for ob in (True, False):
        G = gen(ob)
        x, wt, b = G((n, h, w, 3), 64), G((5, 5, 3, 32), 65), G((32,), 66)
        ref, absum = conv_ref(x, wt, b)
        assert_exact_conditions(absum, ref, ob, what=str(shape))
        c4 = torch.ones((n, h, w, 4), dtype=BF, device=dev)
        c4[..., :3] = dv(x, dev, True)
        c4 = c4.contiguous()
        for act in ('leaky_relu', None):
            full = ref if act is None else lrelu_f32(ref).astype(np.float64)
            want, want_idx = first_max_pool(full)
            pooled, idx = ops.conv1_pool_c4(c4, dv(wt, dev), dv(b, dev), act=act, out_bf16=ob)
            assert_exact(host(pooled), bf16_rne(want) if (ob and act) else want, 'conv1 pooled, act {}'.format(act))
            assert_exact(unpack_argmax2(idx.cpu().numpy()), want_idx, 'conv1 arg-max codes, act {}'.format(act))
        gp = small_ints((n, h // 2, w // 2, 32), 67)
        kk = np.random.default_rng(68).integers(0, 4, size=gp.shape).astype(np.uint8)
        dz = unpool(gp, kk)
        wref, wabs = wgrad_ref(x, dz, 5, 1)
        assert_exact_conditions(wabs, wref, False)
        gd, kd = dv(gp, dev, ob), torch.from_numpy(pack_argmax2(kk)).to(dev)
        dw, db = torch.full((5, 5, 3, 32), 7.0, device=dev), torch.full((32,), 7.0, device=dev)
        ops.conv1_wgrad_c4(c4, gd, kd, dw=dw, db=db)
        assert_exact(host(dw), wref, 'conv1 weight gradient')
        assert_exact(host(db), dz.astype(np.float64).sum(axis=(0, 1, 2)), 'conv1 bias gradient')
        ops.conv1_wgrad_c4(c4, gd, kd, dw=dw, db=db, accumulate=True)
        assert_exact(host(dw), 2 * wref, 'conv1 weight gradient, accumulated')
        wq = small_ints((5, 5, 3, 32), 69)
        dref, dabs = conv_ref(dz, flipped(wq), None)
        assert_exact_conditions(dabs, dref, False)
        assert_exact(host(ops.conv1_dgrad_pooled(gd, kd, dv(wq, dev))), dref, 'conv1 input gradient')
        if ob:      # the generic small-channel forms of the same backward (conv_wgrad_packed_bf16_kernel / conv_dgrad_fewin_bf16_kernel)
            idx8 = torch.from_numpy(kk).to(dev)
            assert_exact(host(ops.conv2d_wgrad_pooled(dv(x, dev), gd, idx8, 5)), wref, 'packed wgrad from the pooled gradient')
            assert_exact(host(ops.conv2d_dgrad_pooled(gd, idx8, dv(wq, dev))), dref, 'few-input dgrad from the pooled gradient')


# ----------------------------------------------------------------------------------------------------------------------
# parity mode (float32 matrix-core kernels: conv_mfma.hip, conv_wgrad.hip, conv_small.hip): the same cases, plus the big kernel
# sizes (even ones have TF's asymmetric SAME padding) and VALID padding
def _f32_case(p):
    c = dict(p.values[0])
    c['ob'], c['xb'], c['zb'] = (False,), False, False
    c.pop('rows', None)
    shape = 'x'.join(str(v) for v in c['shape'])
    c['name'] = 'f32-' + shape + ''.join('-' + k for k in ('pad_mode', 'mask', 'split', 'no_db') if c.get(k))
    return pytest.param(c, id=c['name'])


PARITY_FWD = [_f32_case(p) for p in FWD if 'rows' not in p.values[0] and p.values[0]['shape'][0] <= 8
              and not p.id.startswith(('ring', 'dma'))] + [
    P('k{}-same'.format(k), shape=(2, 19, 22, 3, 0, 8, k, 1), ob=(False,)) for k in (4, 6, 7, 9, 11)] + [
    P('k{}-valid'.format(k), shape=(2, 19, 22, 8, 0, 12, k, 1), ob=(False,), padding='VALID') for k in (1, 3, 4, 5, 6, 7, 9, 11)] + [
    P('k5-s2-valid', shape=(2, 19, 22, 8, 0, 12, 5, 2), ob=(False,), padding='VALID'),
    P('dma4-shape-512to512', shape=(5, 8, 8, 512, 0, 512, 3, 1), ob=(False,)),
    P('fewout-16to3', shape=(2, 16, 16, 16, 0, 3, 3, 1), ob=(False,)),
    P('fewout-32to3-k5', shape=(3, 32, 80, 32, 0, 3, 5, 1), ob=(False,))]


@pytest.mark.parametrize('case', PARITY_FWD)
def test_parity_fwd_exact(dev, case, monkeypatch):
    run_fwd(dev, case, monkeypatch, 'f32')


@pytest.mark.parametrize('case', [_f32_case(p) for p in DGRAD if 'rows' not in p.values[0]])
def test_parity_dgrad_exact(dev, case, monkeypatch):
    case = dict(case)
    if case.get('mask'):
        case['mask'] = 'f32'
    run_dgrad(dev, case, monkeypatch, 'f32')


@pytest.mark.parametrize('case', [_f32_case(p) for p in WGRAD] + [
    P('k{}-big'.format(k), shape=(2, 19, 22, 8, 0, 12, k, 1)) for k in (4, 6, 7, 9, 11)] + [P('k2-s2', shape=(2, 16, 20, 24, 0, 40, 2, 2)),
                                                                                            P('tiny-k3c3', shape=(2, 20, 36, 3, 0, 3, 3, 1), no_db=True)])
def test_parity_wgrad_exact(dev, case):
    if case['shape'][6] == 2:           # the 2x2 / stride-2 form has no padding: it is Conv2DTranspose's weight gradient
        from neural_imaging_amd import ops
        n, h, w, cin, cout = case['shape'][:3] + (case['shape'][3], case['shape'][5])
        x, dy = small_ints((n, h // 2, w // 2, cout), 71), small_ints((n, h, w, cin), 72)
        wtt = torch.zeros((2, 2, cin, cout), dtype=torch.float64, requires_grad=True)
        (T.conv2d_transpose_2x2(to64(x), wtt, None) * to64(dy)).sum().backward()
        assert_exact(host(ops.convt2x2_wgrad(dv(x, dev), dv(dy, dev))), wtt.grad.numpy(), 'convT weight gradient, parity mode')
        return
    run_wgrad(dev, case, 'f32')


# ----------------------------------------------------------------------------------------------------------------------
# 2. impulses: how float32 operands are rounded on their way in, and where each tap lands
F32_ROUTES = [p for p in FWD if not p.values[0].get('xb') and 'rows' not in p.values[0] and not p.values[0].get('pad_mode')]


def shifted(chan, ky, kx, k, s, padding):
    """chan (n, h, w) as tap (ky, kx) of a k x k stride-s convolution sees it: out[y, x] = chan[s y + ky - pad_top, s x + kx - pad_left],
    zero outside the image (TF SAME: the odd padding sample goes after)."""
    n, h, w = chan.shape
    if padding == 'SAME':
        ho, wo = -(-h // s), -(-w // s)
        th, tw = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
        chan = np.pad(chan, ((0, 0), (th // 2, th - th // 2), (tw // 2, tw - tw // 2)))
    else:
        ho, wo = (h - k) // s + 1, (w - k) // s + 1
    return chan[:, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s]


def full_mantissa(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


@pytest.mark.parametrize('case', F32_ROUTES)
def test_impulse_weight_and_pixel(dev, case):
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    n, h, w, c1, c2, cout, k, s = case['shape']
    padding = case.get('padding', 'SAME')
    cin = c1 + c2
    x = full_mantissa((n, h, w, cin), 81)
    xr = bf16_rne(x)
    ci, co = cin - 2, cout - 3
    x1, x2 = dv(x[..., :c1], dev), (dv(x[..., c1:], dev) if c2 else None)
    for ky in range(k):
        for kx in range(k):
            wt = np.zeros((k, k, cin, cout), np.float32)
            wt[ky, kx, ci, co] = 1.0
            chan = shifted(xr[..., ci], ky, kx, k, s, padding)       # a shifted copy of the rounded channel: nothing to sum
            what = 'one-hot weight at tap ({}, {})'.format(ky, kx)
            if (ky, kx) == (k - 1, 0) and x.size <= (1 << 19):       # the shift restated here is the oracle's convolution
                assert_exact(chan, conv_ref(xr, wt, None, s, padding)[0][..., co], 'shifted()')
            out = ops.conv2d(x1, dv(wt, dev), None, x2=x2, stride=s, padding=padding)
            assert tuple(out.shape[:3]) == chan.shape and np.count_nonzero(chan) > 0
            want_d = torch.zeros_like(out)
            want_d[..., co] = torch.from_numpy(chan.astype(np.float32)).to(dev)
            if not torch.equal(out, want_d):                         # (compared on the device; the report is made on the host)
                assert_exact(host(out), host(want_d), what)
    # one-hot pixels in tile corners: the output around each is the rounded kernel, flipped
    wt = full_mantissa((k, k, cin, cout), 82)
    xi = np.zeros((n, h, w, cin), np.float32)
    spots = {(0, 0, 0), (n - 1, h - 1, w - 1), (n - 1, min(h - 1, 15), min(w - 1, 16)), (0, min(h - 1, 8), min(w - 1, 7))}
    for (i, yy, xx) in spots:
        xi[i, yy, xx, (yy + xx) % cin] = 1.0
    want = conv_ref(xi, bf16_rne(wt), None, s, padding)[0]
    got = ops.conv2d(dv(xi[..., :c1], dev), dv(wt, dev), None, x2=dv(xi[..., c1:], dev) if c2 else None, stride=s, padding=padding)
    assert_exact(host(got), want, 'one-hot pixels')


# ----------------------------------------------------------------------------------------------------------------------
# 3. full-mantissa operands, rounded to bf16 first: the float64 oracle sees the same values, only the float32 accumulation differs
MEASURED = []


def check_full_mantissa(name, got, ref, stores_bf16):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    d = np.abs(got - ref)
    if stores_bf16:
        worst = float((d / (2.0 ** -8 * np.abs(ref) + 2e-5 * scale)).max())
        line = 'exact: full mantissa {:<44} bf16 out: max |err| / (2^-8 |ref| + 2e-5 max|ref|) = {:.3f}'.format(name, worst)
    else:
        worst = float(d.max() / scale / 2e-5)
        line = 'exact: full mantissa {:<44} f32 out: max |err| / max|ref| = {:.2e}'.format(name, float(d.max() / scale))
    MEASURED.append(line)
    assert worst <= 1.0, line


@pytest.mark.parametrize('case', [p for p in FWD if 'rows' not in p.values[0] or p.values[0]['rows']])
def test_full_mantissa_fwd(dev, case, monkeypatch):
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout, k, s = case['shape']
    if 'rows' in case:
        monkeypatch.setattr(ops, 'ROWS_CONV', case['rows'])
    ops.set_compute('bf16')
    pad_mode, xb = case.get('pad_mode', 0), case.get('xb', False)
    x, wt, b = bf16_rne(full_mantissa((n, h, w, c1 + c2), 91)), bf16_rne(0.2 * full_mantissa((k, k, c1 + c2, cout), 92)), \
        full_mantissa((cout,), 93)
    padding = case.get('padding', 'SAME')
    ref = conv_ref(x, wt, b, s, padding, pad_mode)[0]
    x1, x2 = dv(x[..., :c1], dev, xb), (dv(x[..., c1:], dev, xb) if c2 else None)
    for ob in case['ob']:
        out = ops.conv2d(x1, dv(wt, dev), dv(b, dev), x2=x2, stride=s, padding=padding, pad_mode=pad_mode, out_bf16=ob)
        check_full_mantissa('fwd[{}]'.format(case['name']), host(out), ref, ob)


@pytest.mark.parametrize('case', [p for p in DGRAD if ('rows' not in p.values[0] or p.values[0]['rows']) and not p.values[0].get('split')])
def test_full_mantissa_dgrad(dev, case, monkeypatch):
    from neural_imaging_amd import ops
    n, h, w, cin, cout, k = case['shape']
    if 'rows' in case:
        monkeypatch.setattr(ops, 'ROWS_CONV', case['rows'])
    ops.set_compute('bf16')
    dz, wt = bf16_rne(full_mantissa((n, h, w, cout), 94)), bf16_rne(0.2 * full_mantissa((k, k, cin, cout), 95))
    ref = conv_ref(dz, flipped(wt), None)[0]
    for ob in case['ob']:
        out = ops.conv2d_dgrad(dv(dz, dev, case.get('zb', False)), dv(wt, dev), (h, w), out_bf16=ob)
        check_full_mantissa('dgrad[{}]'.format(case['name']), host(out), ref, ob)


def test_full_mantissa_summary(dev, capsys):
    """The measured maxima of the routes above in one block of the test log, one line per route (printed past the capture)."""
    assert len(MEASURED) > 0
    with capsys.disabled():
        print('\n'.join(['', 'exact: module wall time so far {:.1f} s'.format(time.monotonic() - _T0[0]),
                         'exact: full-mantissa maxima, one line per route'] + MEASURED), flush=True)
