"""
The cases of tests/test_gpu_tail_exact.py and their REFERENCE HALVES (float64, CPU only): everything between the FAN's last
convolution and the updated weights - loss reductions, bias sums, FAN head, Adam, DCN latent.  Each builder draws the operands,
computes the float64 reference, and asserts - on the reference alone - the conditions under which the comparison means something
(the operand rules of DESIGN.md section 5).  The GPU tests call a builder and compare the kernels with what it returns;
tests/test_tail_helpers.py calls every builder without a GPU.

The loss / gradient divisibility rule (derived, not tuned).  With pixels k / 256 and differences d = j / 256, |j| <= 127:
  mse255   e = 255 d = 255 j / 256 has 15 significant bits, e * e is formed in float64 (30 bits), the float64 sum of n such squares
           is an integer number of 2^-16 below 2^53 (asserted) - exact in ANY order, so loss == float32(s / count).
           gk = gscale * 2 * 255 * 255 / count: the float32 products give gscale * 130050 exactly (17 bits), and the quotient by
           count = 2^e * odd is a float32 number exactly when odd divides 130050 = 2 * 3^2 * 5^2 * 17^2 (any other odd factor gives
           a non-terminating binary fraction).  Then gk * d = gscale * (130050 / odd) * j * 2^-(e + 8): at most 17 + 7 bits - exact,
           and an accumulated gradient r * gk / 256 (small integer r) stays on the same grid: nothing rounds, fused or not.
  mae255   the same with gk = gscale * 255 / count: odd must divide 255 = 3 * 5 * 17; the gradient is +-gk or 0.
  l2_loss  gradient gscale * d: exact for every power-of-two gscale at any count.
"""
from fractions import Fraction

import numpy as np
import torch

from oracle import tables as ot
from oracle import tfops as T

from util import (EXACT_SUM_LIMIT, F32_MIN_NORMAL, F32_UNIT_ROUNDOFF, PIXEL_GRID, assert_exact_conditions, assert_no_denormals,
                  bf16_rne, depth_to_space2, is_f32, mask_f32, odd_part, pack_bits, pixel_pairs, small_ints, space_to_depth2,
                  ternary, to64)

CAP = 2048 * 256                    # grid cap of csrc/common.h grid_for (pointwise, pool, adam, losses): 2048 workgroups of 256
L2CAP = 1024 * 256                  # ... of csrc/latent.hip
BENCH = 64 * 256 * 256 * 3          # the developed batch of the bench's default configuration
F32 = np.float32


def _seed(*parts):
    s = 23
    for p in parts:
        s = (s * 1000003 + (sum(ord(c) for c in p) if isinstance(p, str) else int(p))) % (2 ** 31 - 1)
    return s


# ----------------------------------------------------------------------------------------------------------------------
# loss reductions
GK_CONST = {'mse255': 130050, 'mae255': 255}


def grad_is_exact(kind, count):
    """The divisibility rule of the module docstring."""
    return kind == 'l2_loss' or GK_CONST[kind] % odd_part(count) == 0


def kernel_gk(kind, gscale, count):
    """gk as the kernels compute it, operation by operation in float32."""
    if kind == 'mse255':
        return F32(gscale) * F32(2.0) * F32(255.0) * F32(255.0) / F32(count)
    return F32(gscale) * F32(255.0) / F32(count)


DEEP = {'mse255': 65025 * 32, 'mae255': 65025 * 32, 'l2_loss': 3 * L2CAP + 12345}      # several strides deep, not a multiple of 256
LOSS_CASES = []
for _kind, _cap in (('mse255', CAP), ('mae255', CAP), ('l2_loss', L2CAP)):
    _counts = [1, 63, 64, 65, 255, 256, 257, _cap - 256, _cap, _cap + 1, DEEP[_kind], BENCH]
    if _kind == 'mae255':
        _counts.append(255 * 2 ** 13)                  # the deepest count whose odd part divides 255 (gradient, 3.98 strides)
    for _c in _counts:
        LOSS_CASES.append(dict(name='{}-n{}-loss'.format(_kind, _c), kind=_kind, count=_c, grad=False, acc=False, gscale=1.0))
        if grad_is_exact(_kind, _c):
            LOSS_CASES.append(dict(name='{}-n{}-grad'.format(_kind, _c), kind=_kind, count=_c, grad=True, acc=False, gscale=0.5))
            LOSS_CASES.append(dict(name='{}-n{}-grad-acc'.format(_kind, _c), kind=_kind, count=_c, grad=True, acc=True, gscale=2.0))
assert DEEP['mse255'] % 256 and DEEP['mse255'] > 3 * CAP and grad_is_exact('mse255', DEEP['mse255']) and DEEP['l2_loss'] % 256
assert [grad_is_exact('mse255', n) for n in (5 * 40 * 24 * 3, 3 * 17 * 34 * 3, 15 * 85 * 3, BENCH, 2 * 9 * 50 * 3, 7 * 16 * 16 * 3)] == \
    [True, True, True, True, False, False]


def loss_value(kind, j, count):
    """The float32 loss from the integer differences j (d = j / 256): the float64 sum is exact, then the kernel's own final
    expression restated in numpy float64 and cast once."""
    j = np.asarray(j, np.int64)
    if kind == 'mse255':
        total = int(((255 * j) ** 2).sum())                        # units of 2^-16
        assert total < 2 ** 53, 'the float64 sum of the squares is not exact'
        return F32(np.float64(total) / 65536.0 / np.float64(count))                       # mse255_final_kernel: s / (double)count
    if kind == 'mae255':
        total = int(np.abs(255 * j).sum())                         # units of 2^-8
        assert total < 2 ** 53
        return F32(0.0 + 1.0 * (np.float64(total) / 256.0) * (1.0 / np.float64(count)))   # mean_final_kernel: offset + scale s inv_count
    total = int((j * j).sum())                                     # 0.5 d d: units of 2^-17
    assert total < 2 ** 53
    return F32(np.float64(total) / 131072.0)                       # sum_final_kernel


def loss_case(case):
    kind, count, gscale = case['kind'], case['count'], case['gscale']
    a, b, j = pixel_pairs((count,), _seed('loss', kind, count))
    d = a.astype(np.float64) - b.astype(np.float64)
    assert np.array_equal(d * 256, j) and is_f32(255.0 * d) and is_f32(255.0 * a.astype(np.float64))
    out = dict(a=a, b=b, j=j, loss=loss_value(kind, j, count), grad=None, existing=None)
    assert_no_denormals(a, b, d, [out['loss']], what=case['name'])
    if not case['grad']:
        return out
    assert grad_is_exact(kind, count), case['name'] + ': the gradient scale is not a float32 number at this count'
    if kind == 'l2_loss':
        gk = np.float64(gscale)
        grad, unit = gk * d, gk / 256
    else:
        gk32 = kernel_gk(kind, gscale, count)
        assert Fraction(float(gk32)) == Fraction(gscale) * GK_CONST[kind] / count, 'gk is not exact'
        gk = np.float64(gk32)
        grad, unit = (gk * d, gk / 256) if kind == 'mse255' else (gk * np.sign(j), gk)
        if kind == 'mae255' and count > 300:
            assert (j == 0).any(), 'no zero difference: sign(0) = 0 is not tested'
    assert is_f32(grad), case['name'] + ': gk * d rounds'
    if case['acc']:
        out['existing'] = (small_ints((count,), _seed('acc', kind, count), 3).astype(np.float64) * unit).astype(F32)
        assert is_f32(small_ints((count,), _seed('acc', kind, count), 3).astype(np.float64) * unit)
        grad = out['existing'].astype(np.float64) + grad
        assert is_f32(grad), case['name'] + ': the accumulated gradient rounds - fused and unfused forms would differ'
    assert_no_denormals(grad, [unit], what=case['name'])
    out['grad'] = grad
    return out


# ---- mse255_sum_s2d3: (route, n, h, w, n_parts, gscale); route as nimg_mse255_sum_s2d3 dispatches an aligned call
S2D3_SHAPES = [('rows', 1, 5, 2, 6, 1.0), ('rows-nrows2560', 5, 512, 2, 2, 0.5), ('rows', 1, 2, 510, 3, 1.0), ('rows', 1, 4, 512, 4, 0.125),
               ('rows', 2, 4, 16, 5, 1.0), ('rows-bench-nrows8192', 64, 128, 128, 3, 1.0),
               ('pairs-oddw', 1, 5, 15, 1, 1.0), ('pairs-oddw', 2, 4, 17, 4, 0.5), ('pairs-oddw', 1, 5, 85, 6, 1.0),
               ('pairs-oddw-blocks', 4, 128, 255, 2, 1.0), ('pairs-w514', 1, 2, 514, 3, 1.0)]
S2D3_CASES = [dict(name='s2d3-{}-{}x{}x{}-p{}'.format(r, n, h, w, p), route=r, n=n, h=h, w=w, n_parts=p, gscale=g)
              for r, n, h, w, p, g in S2D3_SHAPES]
S2D3_SWITCH = dict(name='s2d3-2x4x16-p5', route='rows', n=2, h=4, w=16, n_parts=5, gscale=1.0)       # offset operands and the child
S2D3_SWITCH2 = dict(name='s2d3-1x2x510-p3', route='rows', n=1, h=2, w=510, n_parts=3, gscale=1.0)


def s2d3_route(case):
    w = case['w']
    return 'rows' if (w % 2 == 0 and w <= 512) else 'pairs'


def s2d3_case(case):
    """The 12 differences j of every output pixel (a 2 x 2 x 3 quad of the image) are a permutation of {-105, -85, ..., 115} and the
    parts add at most +-6 grid units, so the 12 results of a quad are ALL DISTINCT: a swapped half, pixel or channel is visible.
    Reference: element = float32(gk d + (parts[0] + parts[1] + ...)), the kernel's explicit fmaf - the float64 expression is exact
    (asserted against extended precision), so the single rounding is the kernel's; at the counts that satisfy the divisibility rule
    nothing rounds at all (asserted), and those are all cases but w = 514 (count = 2^4 * 3 * 257)."""
    n, h, w, n_parts, gscale = case['n'], case['h'], case['w'], case['n_parts'], case['gscale']
    assert s2d3_route(case) == case['route'].split('-')[0]
    count = n * h * w * 12
    rng = np.random.default_rng(_seed('s2d3', n, h, w))
    base = np.arange(12) * 20 - 105
    jq = rng.permuted(np.broadcast_to(base, (n * h * w, 12)).copy(), axis=1).reshape(n, h, w, 12)
    a, b, j = pixel_pairs(None, _seed('s2d3ab', n, h, w), j=depth_to_space2(jq))
    d = a.astype(np.float64) - b.astype(np.float64)
    gk32 = kernel_gk('mse255', gscale, count)
    exact = grad_is_exact('mse255', count)
    assert exact == (Fraction(float(gk32)) == Fraction(gscale) * 130050 / count) and (exact or w == 514)
    unit = np.float64(gk32) / 256 if exact else 2.0 ** -12
    parts = [(rng.integers(-1, 2, size=a.shape) * unit).astype(F32) for _ in range(n_parts)]
    acc = parts[0].astype(np.float64)
    for p in parts[1:]:
        acc = acc + p.astype(np.float64)
        assert is_f32(acc)
    img64 = np.float64(gk32) * d + acc
    wide = np.longdouble(gk32) * d.astype(np.longdouble) + acc.astype(np.longdouble)
    assert np.array_equal(wide, img64.astype(np.longdouble)), 'the float64 form of gk d + acc is not exact'
    if exact:
        assert is_f32(img64), case['name'] + ': a qualifying count must not round'
    img = img64.astype(F32)
    ref = space_to_depth2(img)
    assert np.array_equal(ref, T.space_to_depth(torch.from_numpy(img), 2).numpy())
    assert (np.diff(np.sort(ref, axis=-1), axis=-1) > 0).all(), 'a quad with equal values would hide a swap'
    assert_no_denormals(img, a, b, [unit], what=case['name'])
    return dict(a=a, b=b, parts=parts, dz=ref.astype(np.float64), loss=loss_value('mse255', j, count), exact=exact)


# ---- the plain grid-stride kernels: add, add_n, lrelu_bwd
POINT_COUNTS = [1, 255, 257, CAP - 256, CAP, CAP + 1, 3 * CAP + 12345]
ADDN_COUNTS = [4, 1020, 1028, 4 * CAP, 4 * CAP + 4, 9 * CAP + 12]          # the one-pass kernel strides over float4 items


def pointwise_case(count, n):
    xs = [small_ints((count,), _seed('add', count, i), 1000) for i in range(n)]
    ref = np.sum([x.astype(np.float64) for x in xs], axis=0)
    assert_exact_conditions(np.sum([np.abs(x.astype(np.float64)) for x in xs], axis=0), ref, False)
    return xs, ref


def lrelu_bwd_case(count):
    dy, y = small_ints((count,), _seed('lrelu', count), 50), small_ints((count,), _seed('lrelu-y', count), 2)
    assert count < 9 or (y == 0).any()
    return dy, y, mask_f32(dy, y).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# bias_grad / bias_grad_ex
def bias_blocks(npix):
    """(blocks, pixels per block, number of trailing EMPTY blocks) of nimg_bias_grad_ex's block rule."""
    blocks = 1 if npix < 512 else min(npix // 512, 2048)
    ppb = (npix + blocks - 1) // blocks
    return blocks, ppb, blocks - (npix + ppb - 1) // ppb


def bias_route(cout, bf16):
    if bf16:
        return 'bf16'
    return 'float4' if (cout % 4 == 0 and cout // 4 <= 256 and 256 % (cout // 4) == 0) else 'generic'


BIAS_COUTS = [1, 3, 12, 31, 32, 33, 64, 65, 128, 129, 256, 257, 300, 512, 1024]
BIAS_NPIX = [1, 511, 512, 513, 1023, 1025, 2048 * 512 - 1, 2048 * 512 + 1, 2048 * 600 + 7]
BIAS_CASES = [dict(cout=c, npix=p, bf16=False, acc=(c in (3, 64, 300))) for c in BIAS_COUTS for p in (1025, 37)] + \
             [dict(cout=c, npix=p, bf16=False, acc=(p == 513)) for c in (4, 3) for p in BIAS_NPIX] + \
             [dict(cout=c, npix=p, bf16=True, acc=(c == 64)) for c, p in ((4, 2048 * 512 + 1), (4, 513), (32, 1025), (64, 511), (128, 1),
                                                                          (256, 1023), (512, 1025), (1024, 513), (8, 2048 * 600 + 7))
              if bias_route(c, False) == 'float4']
for _c in BIAS_CASES:
    _c['name'] = 'bias-{}-cout{}-npix{}{}'.format(bias_route(_c['cout'], _c['bf16']), _c['cout'], _c['npix'], '-acc' if _c['acc'] else '')


def bias_case(case):
    """npix = 2048 * 512 + 1: 2048 blocks of 513 pixels, blocks 2045 .. 2047 start past the end and sum nothing;
    npix = 2048 * 600 + 7: 2048 blocks of 601, blocks 2045 .. 2047 empty again (asserted below from the block rule)."""
    cout, npix, bf = case['cout'], case['npix'], case['bf16']
    if npix == 2048 * 512 + 1:
        assert bias_blocks(npix) == (2048, 513, 3)
    if npix == 2048 * 600 + 7:
        assert bias_blocks(npix) == (2048, 601, 3)
    seed = _seed('bias', cout, npix, int(bf))
    dz = ternary((npix, cout), seed, 0.5) if bf else small_ints((npix, cout), seed, 3)
    ref = dz.astype(np.float64).sum(axis=0)
    assert_exact_conditions(np.abs(dz.astype(np.float64)).sum(axis=0), ref, False, what=case['name'])
    existing = small_ints((cout,), seed + 1, 100) + F32(0.5) if case['acc'] else None
    if existing is not None:
        assert (existing != 0).all()
        ref = ref + existing
    return dict(dz=dz, existing=existing, ref=ref)


# ----------------------------------------------------------------------------------------------------------------------
# FAN head, generic path
def fan_vector_route(c):
    return c % 4 == 0 and c // 4 <= 256 and 256 % (c // 4) == 0


def fan_parts(n):
    return 1 if n >= 1024 else (4 if n >= 256 else 16)


# (n, hw, c, k): channel routes x hw around parts * ppi, then the classes, then the batch sizes
_FAN = [(5, 16, 4, 5), (5, 64, 32, 5), (5, 256, 64, 5), (5, 16, 256, 5), (5, 64, 256, 5), (5, 256, 256, 5), (5, 16, 1024, 5),
        (5, 64, 1024, 5), (5, 64, 6, 5), (5, 16, 100, 5), (5, 16, 1028, 5), (5, 256, 6, 5)] + \
       [(7, 16, 32, k) for k in (1, 2, 15, 16, 17, 63, 64, 65, 128, 255, 256)] + [(7, 16, 6, k) for k in (16, 17, 256)] + \
       [(n, 16, 32, 5) for n in (1, 255, 256, 1024)] + [(n, 16, 6, 100) for n in (1, 255, 256, 1024)] + \
       [(320, 256, 32, 5), (320, 64, 100, 17), (1024, 64, 32, 17)]
FAN_CASES = [dict(name='fan-{}-n{}-hw{}-c{}-k{}-parts{}'.format('vec' if fan_vector_route(c) else 'scalar', n, hw, c, k, fan_parts(n)),
                  n=n, hw=hw, c=c, k=k) for n, hw, c, k in _FAN]
FAN_HW225 = [dict(name='fan-hw225-{}-c{}'.format('vec' if fan_vector_route(c) else 'scalar', c), n=6, hw=225, c=c, k=5) for c in (32, 6)]


def fan_labels(n, k):
    """class 0, class k - 1 and a class in each 64-lane slot of the wide kernel, cycled over the images (n = 1: class k - 1)."""
    cand = [k - 1, 0] + [s * 64 + 5 for s in range(4) if s * 64 + 5 < k]
    return np.array([cand[i % len(cand)] for i in range(n)], np.int32)


def fan_linear_case(case):
    """The linear parts, exact: gap (small-integer activations, hw a power of two), and the backward with dlogits and loss_per as
    dyadic INPUTS: dw = gap^T dlogits, db = sum dlogits, loss = float32(sum(loss_per) * (double)loss_scale),
    dact = (W dlogits) / hw * LeakyReLU'(act) - one float32 multiply by float32(0.2) where act <= 0 (util.mask_f32)."""
    n, hw, c, k = case['n'], case['hw'], case['c'], case['k']
    assert hw & (hw - 1) == 0
    seed = _seed('fan', n, hw, c, k)
    act = small_ints((n, hw, 1, c), seed, 4)
    assert (act == 0).any() or act.size < 20
    a64 = act.astype(np.float64)
    gap = a64.sum(axis=(1, 2)) / hw
    assert_exact_conditions(np.abs(a64).sum(axis=(1, 2)), gap, False, what=case['name'] + ' gap')
    w = small_ints((c, k), seed + 1, 2)
    dlogits = small_ints((n, k), seed + 2, 4) * F32(2.0 ** -6)
    loss_per = np.random.default_rng(seed + 3).integers(1, 4096, size=n).astype(F32) * F32(2.0 ** -10)
    loss_scale = F32(1.0 / n)
    dw = gap.T @ dlogits.astype(np.float64)
    db = dlogits.astype(np.float64).sum(axis=0)
    unit = 2.0 ** -6 / hw
    assert_exact_conditions(np.abs(gap).T @ np.abs(dlogits.astype(np.float64)), dw, False, scale=unit, what=case['name'] + ' dw')
    assert is_f32(dw) and is_f32(db) and is_f32(gap)
    loss = F32(loss_per.astype(np.float64).sum() * np.float64(loss_scale))
    g = (dlogits.astype(np.float64) @ w.astype(np.float64).T) / hw                               # (n, c)
    assert is_f32(g) and (np.abs(dlogits.astype(np.float64)) @ np.abs(w.astype(np.float64)).T).max() * 64 < EXACT_SUM_LIMIT
    dact = mask_f32(np.broadcast_to(g[:, None, None, :], act.shape), act).astype(np.float64)
    dact_inclusive = mask_f32(np.broadcast_to(g[:, None, None, :], act.shape), act + F32(0.5)).astype(np.float64)    # the wrong `>= 0` rule
    assert_no_denormals(gap, dw, db, dact, dlogits, what=case['name'])
    return dict(act=act, gap=gap, w=w, dlogits=dlogits, loss_per=loss_per, loss_scale=float(loss_scale), dw=dw, db=db, loss=loss,
                dact=dact, dact_inclusive=dact_inclusive, g=g)


def fan_softmax_case(case):
    """Softmax / cross-entropy half against the float64 oracle (expf / logf: tolerances, not ==).  Image 0 carries a feature that
    drives one class's probability above 1 - 1e-7 and every other below 1e-7 (both `inside` branches of the clip are taken: the
    gradient through them is zero)."""
    n, hw, c, k = case['n'], case['hw'], case['c'], case['k']
    rng = np.random.default_rng(_seed('fansm', n, hw, c, k))
    act = rng.uniform(-1, 1, size=(n, hw, 1, c)).astype(F32)
    wt = rng.uniform(-1, 1, size=(c, k)).astype(F32)
    b = rng.uniform(-1, 1, size=(k,)).astype(F32)
    act[0, :, :, 0] = 40.0
    wt[0, :] = -1.0
    wt[0, (k - 1) // 2] = 1.0
    labels = fan_labels(n, k)
    at, wtt, bt = (to64(v).requires_grad_(True) for v in (act, wt, b))
    a = T.leaky_relu(at)
    probs = torch.softmax(a.mean(dim=(1, 2)) @ wtt + bt, dim=1)
    loss = T.sparse_ce_from_probs(probs, labels)
    loss.backward()
    p = probs.detach().numpy()
    if k > 1:
        assert p[0].max() > 1 - 1e-7 and np.sort(p[0])[-2] < 1e-7 and (n == 1 or ((p[1:] > 1e-7) & (p[1:] < 1 - 1e-7)).any())
    return dict(act=a.detach().numpy().astype(F32), w=wt, b=b, labels=labels, probs=p, loss=float(loss.detach()), dw=wtt.grad.numpy(),
                db=bt.grad.numpy(), dact=at.grad.numpy(), gap=a.detach().numpy().mean(axis=(1, 2)))


# ---- fused head (csrc/head.hip): every (hw, c) pair of nimg_head_fused_ok x n in {1, 5, 320}, alpha = 0.25
HEAD_ALPHA = 0.25
HEAD_CASES = [dict(name='head-n{}-hw{}-c{}'.format(n, h * w, c), n=n, h=h, w=w, c=c, zero=False)
              for (h, w) in ((8, 8), (8, 16), (16, 16)) for c in (64, 128, 256) for n in (1, 5, 320)]
HEAD_ZERO_CASE = dict(name='head-zero-rule-n5-hw64-c64', n=5, h=8, w=8, c=64, zero=True)


def head_case(case):
    """Ternary bf16 input and weights, bias = integer + 1/2 (no pre-activation is 0; `zero`: integer bias, zeros occur and must
    CLEAR the bit), alpha = 1/4 (LeakyReLU exact), dlogits / dense weights in {-1, 0, 1} with k = 3: g = A / hw, |A| <= 3, so g
    and alpha g are bf16 numbers and every sum below is an integer number of 1 / (16 hw), far below 2^24 (asserted); the bf16
    results are asserted to be bf16 numbers (at most 8 significant bits)."""
    n, h, w, c, k = case['n'], case['h'], case['w'], case['c'], 3
    hw = h * w
    seed = _seed('head', n, hw, c, int(case['zero']))
    x = ternary((n, h, w, c), seed, 0.25)
    wt = ternary((1, 1, c, c), seed + 1, 8.0 / c)
    b = small_ints((c,), seed + 2, 3) + (F32(0.0) if case['zero'] else F32(0.5))
    x2, w2 = x.reshape(n * hw, c).astype(np.float64), wt.reshape(c, c).astype(np.float64)
    pre = x2 @ w2 + b.astype(np.float64)
    assert_exact_conditions(np.abs(x2) @ np.abs(w2) + np.abs(b), pre, False, scale=0.5, what=case['name'])
    assert (pre == 0).any() == case['zero'], case['name'] + ': zeros among the pre-activations'
    pos = pre > 0
    act = np.where(pos, pre, HEAD_ALPHA * pre)
    gap = act.reshape(n, hw, c).sum(axis=1) / hw
    assert_exact_conditions(np.abs(act).reshape(n, hw, c).sum(axis=1), gap, False, scale=0.125, what=case['name'] + ' gap')
    mask = pack_bits(pos.reshape(n * hw, c // 32, 32))
    mask_p = pack_bits(pos.reshape(n, hw // 32, 32, c).transpose(0, 1, 3, 2))
    mask_inclusive = pack_bits((pre >= 0).reshape(n * hw, c // 32, 32))
    dlogits, wd = small_ints((n, k), seed + 3, 1), small_ints((c, k), seed + 4, 1)
    g = (dlogits.astype(np.float64) @ wd.astype(np.float64).T) / hw                               # (n, c)
    dact = np.repeat(g, hw, axis=0) * np.where(pos, 1.0, HEAD_ALPHA)                             # (n hw, c)
    assert np.array_equal(bf16_rne(dact.astype(F32)), dact)
    unit = 1.0 / (16 * hw)
    dw = x2.T @ dact
    db = dact.sum(axis=0)
    assert_exact_conditions(np.abs(x2).T @ np.abs(dact), dw, False, scale=unit, what=case['name'] + ' dw')
    assert_exact_conditions(np.abs(dact).sum(axis=0), db, False, scale=unit, what=case['name'] + ' db')
    dw0, db0 = small_ints((c, c), seed + 5, 9) * F32(unit * 16), small_ints((c,), seed + 6, 9) * F32(unit * 16)
    dx_nomask = dact @ w2.T
    assert_exact_conditions(np.abs(dact) @ np.abs(w2).T, dx_nomask, False, scale=unit, what=case['name'] + ' dx')
    dx = dx_nomask * np.where(x2 > 0, 1.0, HEAD_ALPHA)
    for name, v in (('dx', dx), ('dx without in_mask', dx_nomask)):
        assert np.array_equal(bf16_rne(v.astype(F32)), v), '{}: {} is not a bf16 tensor'.format(case['name'], name)
    assert_no_denormals(gap, dact, dw, db, dx, what=case['name'])
    return dict(x=x, w=wt, b=b, pre=pre, gap=gap, mask=mask, mask_p=mask_p, mask_inclusive=mask_inclusive, dlogits=dlogits, wd=wd,
                dact=dact.reshape(n, h, w, c), dw=dw, db=db, dw0=dw0, db0=db0, dx=dx.reshape(n, h, w, c),
                dx_nomask=dx_nomask.reshape(n, h, w, c))


# ----------------------------------------------------------------------------------------------------------------------
# Adam
def adam_lr_t64(lr, step, b1, b2):
    """The host's float64 expression (nimg_adam_step / ops.adam_lr_t) on the float32 values that cross the C ABI."""
    lr, b1, b2 = (float(F32(v)) for v in (lr, b1, b2))
    return lr * np.sqrt(1.0 - b2 ** float(step)) / (1.0 - b1 ** float(step))


def adam_reference(p0, grads, lr, b1, b2, eps, gscale=1.0, first_step=1, bug=None):
    """float64 Adam over len(grads) steps with a per-element RUNNING ERROR BOUND of the float32 kernel.  Unit roundoff u = 2^-24;
    every float32 operation of adam_kernel contributes u * (|its result| + the error already carried by its operands):

      gi = gscale * g                         1 rounding (none when gscale is a power of two: asserted by the callers that need it)
      mi = b1 * m + (1 - b1) * gi             3 roundings: the two products and the sum (1.0f - b1 is exact for 0.5 <= b1 <= 1,
                                              Sterbenz; a contraction to fma only removes roundings) + b1 E(m) + (1 - b1) E(gi)
      vi = b2 * v + ((1 - b2) * gi) * gi      4 roundings: three products and the sum + b2 E(v) + (1 - b2) (2 |gi| + E(gi)) E(gi)
      upd = lr_t * mi / (sqrtf(vi) + eps)     5 roundings: the float cast of lr_t, lr_t * mi, sqrtf, + eps and the division
                                              (IEEE-correct division and square root: no fast-math flag in the build); the carried
                                              errors go through the quotient rule with the denominator's lower bound, and through
                                              sqrt by its concavity: |sqrt(v') - sqrt(v)| <= sqrt(v) - sqrt(max(v - E(v), 0))
      p -= upd                                1 rounding: u |p|, + E(upd)
    Errors carry additively over the steps.  Returns p, m, v and Ep, Em, Ev (all float64).  bug: the wrong formulas of the
    self-test ('eps_inside', 'no_eps', 'step_minus_1', 'betas_swapped') - then the float32 stand-in, no bound."""
    u = F32_UNIT_ROUNDOFF
    b1, b2, eps, gs = (np.float64(F32(v)) for v in (b1, b2, eps, gscale))
    assert 0.5 <= b1 <= 1 and 0.5 <= b2 <= 1
    p, m, v = np.asarray(p0, np.float64).copy(), np.zeros(len(p0)), np.zeros(len(p0))
    Ep, Em, Ev = np.zeros(len(p0)), np.zeros(len(p0)), np.zeros(len(p0))
    for t, g in enumerate(grads):
        step = first_step + t
        g = np.asarray(g, np.float64)
        gi = gs * g
        Eg = np.zeros_like(gi) if odd_part_is_one(gs) else u * np.abs(gi)
        rnd = lambda x, e: e + u * (np.abs(x) + e)                    # one float32 rounding of a value x carrying the error e
        m1, m2 = b1 * m, (1.0 - b1) * gi
        m_new = m1 + m2
        Em = rnd(m_new, rnd(m1, b1 * Em) + rnd(m2, (1.0 - b1) * Eg))
        v1, v2 = b2 * v, (1.0 - b2) * gi
        E2 = rnd(v2, (1.0 - b2) * Eg)
        v3 = v2 * gi
        E3 = rnd(v3, np.abs(gi) * E2 + np.abs(v2) * Eg + E2 * Eg)
        v_new = v1 + v3
        Ev = rnd(v_new, rnd(v1, b2 * Ev) + E3)
        m, v = m_new, v_new
        lr_t = adam_lr_t64(lr, step, b1, b2)
        num, root = lr_t * m, np.sqrt(v)
        den = root + eps
        E_num = lr_t * Em + 2 * u * (np.abs(num) + lr_t * Em)
        d_root = root - np.sqrt(np.maximum(v - Ev, 0.0)) + u * root
        E_den = d_root + u * (den + d_root)
        assert (den - E_den > 0).all()
        upd = num / den
        E_upd = E_num / (den - E_den) + np.abs(num) * E_den / (den * (den - E_den))
        E_upd = E_upd + u * (np.abs(upd) + E_upd)
        p = p - upd
        Ep = Ep + E_upd + u * (np.abs(p) + Ep + E_upd)
    return p, m, v, Ep, Em, Ev


def odd_part_is_one(x):
    m, _ = np.frexp(float(x))
    return m == 0.5


def adam_f32(p0, grads, lr, b1, b2, eps, gscale=1.0, first_step=1, bug=None):
    """float32 numpy stand-in of adam_kernel, operation by operation (bug: the wrong variants of the self-test)."""
    b1, b2, eps, gs = F32(b1), F32(b2), F32(eps), F32(gscale)
    p, m, v = np.array(p0, F32), np.zeros(len(p0), F32), np.zeros(len(p0), F32)
    one = F32(1.0)
    with np.errstate(all='ignore'):
        for t, g in enumerate(grads):
            step = first_step + t - (1 if bug == 'step_minus_1' else 0)
            lr_t = F32(adam_lr_t64(lr, step, b2, b1) if bug == 'betas_swapped' else adam_lr_t64(lr, step, b1, b2))
            gi = gs * np.asarray(g, F32)
            m = b1 * m + (one - b1) * gi
            v = b2 * v + (one - b2) * gi * gi
            if bug == 'eps_inside':
                den = np.sqrt(v + eps)
            elif bug == 'no_eps':
                den = np.sqrt(v)
            else:
                den = np.sqrt(v) + eps
            p = p - lr_t * m / den
    return p, m, v


def adam_populations(count, seed):
    """(p0, grads of 5 steps): four interleaved populations - gradients of order 1; |g| in 2^-40 .. 2^-20 (sqrt(v) is far below eps,
    eps decides the update; parameters of order 2^-10 so the bound stays below the effect); exactly 0 throughout (the parameter must
    not move by a bit); mixed signs step to step."""
    rng = np.random.default_rng(seed)
    pop = np.arange(count) % 4
    p0 = rng.uniform(-1, 1, size=count)
    p0 = np.where(pop == 1, p0 * 2.0 ** -10, p0).astype(F32)
    grads = []
    for _ in range(5):
        g = rng.uniform(0.25, 1.0, size=count)
        tiny = g * 2.0 ** rng.integers(-40, -19, size=count)
        sign = np.where(rng.random(count) < 0.5, -1.0, 1.0)
        grads.append(np.select([pop == 0, pop == 1, pop == 2], [g, tiny, 0.0], g * sign).astype(F32))
    return p0, grads, pop


ADAM_COUNTS = [1, 255, 257, CAP, CAP + 1, 3 * CAP + 12345]
ADAM_RATES = [1e-4, 1e-3]                  # the workflows' learning rates (manipulation classification, NIP / DCN training)


def adam_tier1_case(count, gscale):
    """b1 = 1/2, b2 = 3/4, gradients i * 2^-k with |i| <= 3: after 3 steps m is a multiple of 2^-(k + 4) and v of 2^-(2 k + 8) with
    a numerator of at most 12 bits - float32 numbers, whatever the contraction (asserted)."""
    rng = np.random.default_rng(_seed('adam1', count))
    p0 = (rng.integers(-512, 513, size=count) * 2.0 ** -9).astype(F32)
    grads = [(rng.integers(-3, 4, size=count) * 2.0 ** -rng.integers(0, 6, size=count)).astype(F32) for _ in range(3)]
    ref = adam_reference(p0, grads, 1e-3, 0.5, 0.75, 1e-7, gscale)
    assert is_f32(ref[1]) and is_f32(ref[2])
    m, v, gs = np.zeros(count), np.zeros(count), float(gscale)
    for g in grads:                                                    # ... and so is every intermediate: nothing rounds
        gi = gs * g.astype(np.float64)
        steps = [gi, 0.5 * m, 0.5 * gi, 0.75 * v, 0.25 * gi, 0.25 * gi * gi]
        m, v = 0.5 * m + 0.5 * gi, 0.75 * v + 0.25 * gi * gi
        assert all(is_f32(t) for t in steps + [m, v])
        assert_no_denormals(*steps, what='adam tier 1')
    assert np.array_equal(m, ref[1]) and np.array_equal(v, ref[2])
    assert_no_denormals(ref[1], ref[2], *grads, what='adam tier 1')
    return p0, grads, ref


def adam_tier2_case(count, lr, gscale=1.0):
    p0, grads, pop = adam_populations(count, _seed('adam2', count))
    ref = adam_reference(p0, grads, lr, 0.9, 0.999, 1e-7, gscale)
    assert_no_denormals(ref[1], ref[2], *grads, what='adam tier 2')
    if count >= 8:
        root = np.sqrt(ref[2][pop == 1])
        assert (root < 1e-7).all() and (root > 0).all(), 'population 2: sqrt(v) must stay below eps'
    return p0, grads, ref, pop


def assert_within_bound(got, ref, bound, what=''):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    bad = ~(np.abs(got - ref) <= bound)
    if bad.any():
        i = int(np.argmax(np.where(bad, np.abs(got - ref) - bound, -np.inf)))
        raise AssertionError('{}: {} of {} elements outside the running error bound; worst at {}: got {!r}, want {!r}, bound {:.3e}'.format(
            what, int(bad.sum()), got.size, i, float(got[i]), float(ref[i]), float(bound[i])))


NAN_CASES = [('first', 3 * CAP + 12345, 0, 1), ('last', 3 * CAP + 12345, -1, 1), ('tail-past-the-cap', 3 * CAP + 12345, 3 * CAP + 7, 1),
             ('small-last', 257, -1, 1), ('inf-only', CAP + 1, None, 0), ('clean', 255, None, 0)]


# ----------------------------------------------------------------------------------------------------------------------
# DCN latent
LAT_TOL = dict(latent=1e-5, entropy=1e-5, dz=(1e-6, 2e-4), dscale=2e-4)       # test_latent_soft_codebook_and_entropy
CONFIG3 = 50 * 16 * 16 * 32                                                 # the latent of the codec's training batch (bench c3)


def unit_codebook(K):
    return (np.arange(K) - (K // 2 - 1)).astype(F32)


def latent_route(K, v, unit, soft=True):
    """The row of nimg_latent_fwd's / _bwd's dispatch table."""
    m = v + 1
    fast = K in (8, 16, 32) and v > 0 and m <= 1024 and m == int(m)
    if not fast:
        return 'generic{}'.format(64 if K <= 64 else (128 if K <= 128 else 256))
    if unit and m == 51:
        return 'win{}'.format(K)
    return 'fast{}-m{}'.format(K, 51 if m == 51 else 'int')


_LAT = [(K, v, unit) for K in (8, 16, 32) for (v, unit) in ((50.0, True), (50.0, False), (2.0, False))] + \
       [(32, 2.5, False)] + [(K, 50.0, False) for K in (5, 64, 65, 128, 129, 256)]
LATENT_CASES = [dict(name='latent-{}-K{}-v{}-n{}'.format(latent_route(K, v, unit), K, v, 1500 if K <= 64 else 600), K=K, v=v, unit=unit,
                     count=1500 if K <= 64 else 600, cb='unit', scale=1.3) for K, v, unit in _LAT] + \
               [dict(name='latent-fast8-m51-nonunit-codebook', K=8, v=50.0, unit=False, count=1500, cb='x1.5', scale=0.7),
                dict(name='latent-win32-scale-null', K=32, v=50.0, unit=True, count=1500, cb='unit', scale=None),
                dict(name='latent-fast32-m51-scale-null', K=32, v=50.0, unit=False, count=1500, cb='unit', scale=None)] + \
               [dict(name='latent-win32-n{}'.format(n), K=32, v=50.0, unit=True, count=n, cb='unit', scale=1.3)
                for n in (1, 255, L2CAP, L2CAP + 1, CONFIG3)]
LATENT_PROBE_CASES = [dict(name='latent-win{}-probe'.format(K), K=K, v=50.0, unit=True, cb='unit', scale=None) for K in (8, 16)]
LATENT_ROUNDING_CASES = [dict(name='latent-rounding-{}'.format(r), rounding=r, K=32) for r in ('identity', 'soft', 'sin')]
LATENT_SWITCH = dict(name='latent-switch-K32', K=32, v=50.0, unit=True, count=1500, cb='unit', scale=1.3)


def _away_from_midpoints(z, scale, cb, rng, width=1e-4):
    """Redraw (on the CPU) the inputs whose scaled value lies within `width` of a midpoint between two centres: the hard index is
    then the same in float32 and float64."""
    mids = (cb[:-1].astype(np.float64) + cb[1:].astype(np.float64)) / 2
    for _ in range(100):
        zs = (z * F32(scale)).astype(np.float64)
        bad = (np.abs(zs[:, None] - mids[None, :]) <= width).any(axis=1)
        if not bad.any():
            return z
        z[bad] = rng.uniform(cb[0] - 1, cb[-1] + 1, size=int(bad.sum())).astype(F32) / F32(scale)
    raise AssertionError('could not move every input away from the midpoints')


def f32_product(zt, st):
    """z * scale as the reference layer forms it (layers.py:197-198: a float32 product): the oracle is evaluated AT the float32
    product, its derivatives are those of the product.  One float32 rounding of a value near 129 (K = 256) is 2^-18, and through
    the soft codebook's slope (gamma = 25) that alone moves dz by 2e-4 of its maximum - the float64 product is not the reference."""
    prod = zt * st
    zs32 = (zt.detach().to(torch.float32) * st.detach().to(torch.float32)).to(torch.float64)
    return prod + (zs32 - prod).detach()


def latent_reference(z, scale, cb, v, gamma=25.0, coef=250.0, dl=None):
    """(latent, entropy, dz, dscale) of the float64 oracle on the float32 product z * scale (f32_product)."""
    s32 = F32(1.0 if scale is None else scale)
    zt = to64(z).requires_grad_(True)
    st = torch.tensor(float(s32), dtype=torch.float64, requires_grad=True)
    lat = T.soft_codebook(f32_product(zt, st), to64(cb), v=v, gamma=gamma)
    ent, hist = T.entropy(lat, to64(cb), v=v, gamma=gamma)
    ((lat * to64(dl)).sum() + coef * ent).backward()
    return lat.detach().numpy(), float(ent.detach()), zt.grad.numpy(), float(st.grad), hist.detach().numpy()


def latent_case(case):
    K, v, count, scale = case['K'], case['v'], case['count'], case['scale']
    cb = unit_codebook(K) if case['cb'] == 'unit' else (unit_codebook(K) * F32(1.5))
    assert latent_route(K, v, case['unit']) in case['name'] or 'switch' in case['name']
    rng = np.random.default_rng(_seed('latent', K, int(10 * v), count))
    s = 1.0 if scale is None else scale
    z = (rng.uniform(cb[0] - 1.5, cb[-1] + 1.5, size=count) / s).astype(F32)
    z = _away_from_midpoints(z, s, cb, rng)
    dl = rng.uniform(-1, 1, size=count).astype(F32)
    lat, ent, dz, dscale, _ = latent_reference(z, scale, cb, v, dl=dl)
    return dict(z=z, cb=cb, dl=dl, latent=lat, entropy=ent, dz=dz, dscale=dscale)


def latent_probe_case(case):
    """The probe of test_latent_soft_codebook_and_entropy at K = 8 / 16 (the five-centre window touches both ends of the codebook):
    centres, midpoints + 1e-4 / - 1e-4, both range ends, just outside and far outside (there the full loop runs)."""
    K = case['K']
    cb = unit_codebook(K)
    mids = cb[:-1] + 0.5
    z = np.concatenate([cb, mids + 1e-4, mids - 1e-4, [cb[0] - 0.4999, cb[0] - 0.51, cb[-1] + 0.4999, cb[-1] + 0.6, -40.0, 55.0, cb[0] - 3.0],
                        np.random.default_rng(K).uniform(-K, K, size=400)]).astype(F32)
    z = _away_from_midpoints(z, 1.0, cb, np.random.default_rng(K + 1), width=5e-5)
    dl = np.random.default_rng(K + 2).uniform(-1, 1, size=z.shape).astype(F32)
    lat, ent, dz, dscale, _ = latent_reference(z, None, cb, 50.0, dl=dl)
    return dict(z=z, cb=cb, dl=dl, latent=lat, entropy=ent, dz=dz, dscale=dscale)


def latent_rounding_case(case):
    """soft_codebook = False: latent = quantization(scale z, mode) (identity | soft | sin), entropy of that, d/dz through the
    sinusoidal derivative.  Inputs within 1e-4 of a half-integer are redrawn (tf.round would be ambiguous)."""
    K, mode = case['K'], case['rounding']
    cb = unit_codebook(K)
    rng = np.random.default_rng(_seed('round', mode))
    scale = F32(1.3)
    z = (rng.uniform(-8, 8, size=1500) / scale).astype(F32)
    for _ in range(100):
        zs = (z * scale).astype(np.float64)
        bad = np.abs(zs - np.floor(zs) - 0.5) <= 1e-4
        if not bad.any():
            break
        z[bad] = (rng.uniform(-8, 8, size=int(bad.sum())) / scale).astype(F32)
    dl = rng.uniform(-1, 1, size=z.shape).astype(F32)
    zt = to64(z).requires_grad_(True)
    st = torch.tensor(float(scale), dtype=torch.float64, requires_grad=True)
    lat = T.quantization(f32_product(zt, st), mode)
    ent, _ = T.entropy(lat, to64(cb))
    ((lat * to64(dl)).sum() + 250.0 * ent).backward()
    return dict(z=z, cb=cb, dl=dl, scale=float(scale), latent=lat.detach().numpy(), entropy=float(ent.detach()), dz=zt.grad.numpy(),
                dscale=float(st.grad))


HIST_BLOCKS = [1, 15, 16, 17, 1024]


def hist_entropy(counts):
    """-sum q ln q / 0.6931 of a hard histogram with tf_helpers.entropy's clip at 1e-9 and renormalisation."""
    h = np.maximum(np.asarray(counts, np.float64) / np.sum(counts), 1e-9)
    q = h / h.sum()
    return float(-(q * np.log(q)).sum() / 0.6931)


def hist_case(nblocks, K=32, drop_block=None):
    """z EXACTLY on the centres, centre k occurring k + 1 times per 528 = sum(k + 1) values, SORTED, count chosen so the kernels
    launch `nblocks` workgroups (1024: 264000 values, more than 1024 workgroups' worth): every normalised weight is 1 at its own
    centre and below 1e-29 elsewhere, so the entropy is the closed form of the hard histogram.  drop_block: the closed form of a
    histogram that lost the values of one workgroup (the wrong stand-in of the self-test)."""
    cb = unit_codebook(K)
    count = {1: 200, 15: 15 * 256, 16: 16 * 256 - 3, 17: 16 * 256 + 1, 1024: 528 * 500}[nblocks]
    assert min((count + 255) // 256, 1024) == nblocks
    pattern = np.repeat(np.arange(K), np.arange(K) + 1)
    idx = np.tile(pattern, count // len(pattern) + 1)[:count]
    idx = np.sort(idx)                          # sorted: a workgroup sees one or two centres only, so a lost partial moves the entropy
    counts = np.bincount(idx, minlength=K).astype(np.float64)
    if drop_block is not None:
        grid = nblocks * 256
        lost = idx[np.arange(count) % grid // 256 == drop_block]
        counts = counts - np.bincount(lost, minlength=K)
    return dict(z=cb[idx], cb=cb, entropy=hist_entropy(counts), idx=idx)
