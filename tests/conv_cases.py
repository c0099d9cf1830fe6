"""
Cases, operands and float64 references of tests/test_gpu_conv_switches.py, shared with its children (tests/conv_child.py) and with
the CPU self-test (tests/test_conv_switch_helpers.py).  Nothing here needs a GPU except run(), which the children (and the
in-process tests of the per-call switches) call with the bound `ops` module.

SWITCHES is the inventory of every getenv("NIMG_...") read under csrc/: the self-test scans the sources and fails when the two
disagree.  GROUPS maps a child-process group to the environment it runs in and the cases it runs.  A case is a dict: `kind` names
the ops call, `name` the key prefix of its result tensors in the child's .npz, the rest the shape and the operand storage.  The
operands follow tests/test_gpu_exact.py: util.ternary where the output is stored as bf16, util.small_ints otherwise, so every result
is an integer that float32 sums hold exactly in ANY order - `==` against the float64 oracle; `full=True` cases carry full-mantissa
operands rounded to bf16 first and are held to check_full()'s tolerances (the ones of test_full_mantissa_*).
"""
import functools
import os

import numpy as np
import torch

from oracle import tfops as T

from util import (assert_exact_conditions, bf16_rne, first_max_pool, lrelu_f32, mask_f32, small_ints, ternary, to64, unpool)

PAD_NAMES = {1: 'SYMMETRIC', 2: 'REFLECT'}
BIG = '4096'                       # a split-K target no shape here reaches: the slab count is bounded by the work and the workspace

# ----------------------------------------------------------------------------------------------------------------------
# the inventory: name -> status ('group:<g>[,<g>]' | 'per_call' | 'covered_elsewhere:<module>' | 'excluded:<reason>')
SWITCHES = {
    # conv_bf16_tile.h
    'NIMG_NO_BUFFER_LOADS': 'group:plain',
    'NIMG_NO_CONV3_DMA': 'group:fallbacks',
    'NIMG_NO_CONV5_RING': 'group:fallbacks',
    'NIMG_NO_CK64': 'group:fallbacks',
    'NIMG_TN32_BELOW': 'group:plain,fallbacks,optin_a,optin_b,tickets_splits',
    'NIMG_CONV3_RING_MIN': 'group:optin_a',
    'NIMG_NO_CONV5_RING64': 'group:optin_a',          # (not beside NIMG_RING_TN64: it would mask the ring64 route that one opens)
    'NIMG_RING_TN64': 'group:optin_b',
    'NIMG_NO_CONV5_RING32': 'group:optin_b',
    'NIMG_CONV3_DMA_MAXHW': 'group:splits',
    # conv_bf16_ring.h, conv_bf16_dma.h
    'NIMG_RING_NW8': 'group:optin_a',
    'NIMG_CONV3_PLANES': 'group:optin_a',
    'NIMG_CONV3_STAGES': 'excluded:compiled out of the default build (#ifdef NIMG_CONV3_VARIANTS, tools/build_variant.sh only)',
    'NIMG_CONV3_PIPE': 'excluded:compiled out of the default build (#ifdef NIMG_CONV3_VARIANTS, tools/build_variant.sh only)',
    'NIMG_CONV3_ILV': 'excluded:compiled out of the default build (#ifdef NIMG_CONV3_VARIANTS, tools/build_variant.sh only)',
    'NIMG_CONV3_LOADER': 'excluded:compiled out of the default build (#ifdef NIMG_CONV3_VARIANTS, tools/build_variant.sh only)',
    # conv_bf16.hip
    'NIMG_NO_CONVT_FAT': 'group:fallbacks',
    # conv_bf16_wgrad.hip
    'NIMG_NO_WGRAD_PAIR8': 'group:fallbacks',
    'NIMG_NO_NARROW_WGRAD': 'group:fallbacks',
    'NIMG_WGRAD5_BLOCKS': 'group:splits',
    # wgrad3.hip, wgrad5.hip, dgrad5s.hip
    'NIMG_WGRAD3_BLOCKS': 'group:splits,tickets_splits',
    'NIMG_NO_WGRAD3_ALLTAPS': 'per_call',
    'NIMG_WGRAD3_NB': 'per_call',
    'NIMG_WGRAD5_W4': 'per_call',
    'NIMG_NO_WGRAD5_SPARSE': 'per_call',
    'NIMG_WGRAD5_ALLTAPS_BLOCKS': 'group:splits',
    'NIMG_NO_WGRAD5_ALLTAPS': 'group:fallbacks',
    'NIMG_WGRAD5_TH8': 'group:optin_a',
    'NIMG_WGRAD5_KX3L': 'group:optin_a,optin_b,no_tickets',
    'NIMG_WGRAD5_SCHED': 'group:optin_a,optin_b,splits',
    'NIMG_DGRAD5S_ACC16': 'group:optin_a',
    'NIMG_DGRAD5S_BLOCK42': 'group:optin_b',
    # conv_small.hip, frontend.hip, conv3_rows.hip
    'NIMG_NO_C3K5_MFMA': 'group:fallbacks',
    'NIMG_C3K5_TR8': 'group:optin_b',
    'NIMG_CCONV_VARIANT': 'group:optin_b',
    'NIMG_CCONV_CAP': 'group:splits',
    'NIMG_CONV1_CAP': 'group:splits',
    'NIMG_C5C3_ABL': 'excluded:ablation of conv5c3_mfma_kernel for timing, leaves parts of the layer out by design',
    'NIMG_ROWS_ABLATE': 'excluded:ablation of conv3_rows_kernel for timing, leaves parts of the layer out by design',
    'NIMG_ROWS_RB': 'excluded:dead read, the value is (void)-ed and selects nothing',
    'NIMG_ROWS_WGS': 'group:splits',
    'NIMG_ROWS_BH': 'group:splits',
    'NIMG_ROWS_NCW': 'group:splits,optin_b',
    'NIMG_ROWS_PFD': 'group:optin_b',
    # runtime.hip
    'NIMG_NO_TICKETS': 'group:no_tickets',
    # other kernel families
    'NIMG_NO_S2D3_ROWS': 'covered_elsewhere:test_gpu_tail_exact',
    'NIMG_LATENT_GENERIC': 'covered_elsewhere:test_gpu_tail_exact',
    'NIMG_LATENT_GENERIC_POW': 'covered_elsewhere:test_gpu_tail_exact',
    'NIMG_LATENT_NO_WINDOW': 'covered_elsewhere:test_gpu_tail_exact',
    'NIMG_GAUSS_NARROW': 'covered_elsewhere:test_gpu_chain_exact',
    'NIMG_SPARSE_AXIS_SCALAR': 'covered_elsewhere:test_gpu_chain_exact',
}
PER_CALL = ('NIMG_NO_WGRAD3_ALLTAPS', 'NIMG_WGRAD3_NB', 'NIMG_WGRAD5_W4', 'NIMG_NO_WGRAD5_SPARSE')


# ----------------------------------------------------------------------------------------------------------------------
# restatement of the split-K plans (conv_bf16_wgrad.hip splits_for, wgrad3.hip launch, common.h ticket_group): chooses the ticket shapes
def cdiv(a, b):
    return -(-a // b)


def splits_for(cin, cout, n, hout, wout, th=8, target=512):
    blocks_io = cdiv(cin, 32) * cdiv(cout, 64)
    work = n * cdiv(hout, th) * cdiv(wout, 16)
    splits = max(1, min(cdiv(target, blocks_io), work))
    wps = cdiv(work, splits)
    return cdiv(work, wps)


def generic_splits(case, wgrad5_blocks=256):
    """Slabs of conv_wgrad_bf16_kernel for a 'wgrad' case (not its pair8 form)."""
    n, h, w, c1, c2, cout, k, s = case['shape']
    ho, wo = cdiv(h, s), cdiv(w, s)
    k5 = s == 1 and k == 5
    return splits_for(c1 + c2, cout, n, ho, wo, 16 if k5 else 8, min(512, max(32, wgrad5_blocks)) if k5 else 512)


def pair8_splits(case):
    n, h, w, c1, c2, cout, k, s = case['shape']
    pairs = (n + 1) // 2
    sp = min(generic_splits(case), pairs)
    return cdiv(pairs, cdiv(pairs, sp))


def alltaps3_plan(case, target=256):
    """(NB, TH, slabs) of conv3_wgrad_alltaps_kernel for a 'wgrad' case, or None when the shape is not that kernel's."""
    n, h, w, c1, c2, cout, k, s = case['shape']
    if k != 3 or s != 1 or not (case.get('xb') and case.get('zb')) or c1 % 32 or c2 % 32 or cout % 32 or w % 16 or h % 8:
        return None
    nb = int((case.get('env') or {}).get('NIMG_WGRAD3_NB', 0))
    if nb not in (1, 2, 4):
        nb = 4 if cout % 128 == 0 else (2 if cout % 64 == 0 else 1)
    while nb > 1 and cout % (32 * nb):
        nb >>= 1
    th = 16 if (nb == 1 and h % 16 == 0) else 8
    work = n * (h // th) * (w // 16)
    blocks_io = ((c1 + c2) // 32) * (cout // (32 * nb))
    splits = min(cdiv(target, blocks_io), splits_for(c1 + c2, cout, n, h, w), work)
    return nb, th, cdiv(work, cdiv(work, splits))


def ticket_group(splits):
    if splits <= 24:
        return max(1, splits)
    g = 1
    while g * g < splits:
        g += 1
    return g


def ticket_slabs(case, wgrad3_blocks=256):
    """Slabs the ticket finish sums for a 'wgrad' case of the ticket groups."""
    n, h, w, c1, c2, cout, k, s = case['shape']
    plan = alltaps3_plan(case, wgrad3_blocks)
    if plan is not None:
        return plan[2]
    if k == 3 and s == 1 and h == 8 and w == 8 and case.get('xb') and case.get('zb') and n >= 2:
        return pair8_splits(case)
    return generic_splits(case)


# ----------------------------------------------------------------------------------------------------------------------
# case constructors
def _c(kind, name, **kw):
    kw.update(kind=kind, name=name)
    return kw


def fwd(name, shape, ob, xb=True, **kw):
    """shape = (n, h, w, c1, c2, cout, k, stride): ops.conv2d, without and with LeakyReLU."""
    return _c('fwd', name, shape=shape, ob=ob, xb=xb, **kw)


def dgrad(name, shape, ob, zb=True, **kw):
    """shape = (n, h, w, cin, cout, k): ops.conv2d_dgrad, plain and x LeakyReLU' of a mask stored like dz."""
    return _c('dgrad', name, shape=shape, ob=ob, zb=zb, **kw)


def pool(name, shape, ob, **kw):
    """shape = (n, h, w, cin, cout, k): ops.conv2d_pool - pooled values and every arg-max byte, with and without LeakyReLU
    (lrelu_only: the 384-workgroup cases, whose results are 3 MB each).  nimg_conv2d_fwd_pool_bf16 takes the 32-channel tile below
    384 workgroups of 64 channels whatever NIMG_TN32_BELOW says, so the 64-channel tiles and the rings need that many."""
    return _c('pool', name, shape=shape, ob=ob, **kw)


def and_pool(name, shape, **kw):
    """shape = (n, h, w, cin, cout): ops.conv2d_and_pool (pool_also epilogue)."""
    return _c('and_pool', name, shape=shape, **kw)


def dgrad_unpool(name, shape, ob, sparse=False, fold=True, **kw):
    """shape = (n, h, w, cin, cout): 5x5 input gradient from (pooled gradient, arg-max bytes).  fold=False: unpool_fold_ok must say
    no, and the materialising form (maxpool2_unpool, then conv2d_dgrad) runs, as in models/forensics.py."""
    return _c('dgrad_unpool', name, shape=shape, ob=ob, sparse=sparse, fold=fold, **kw)


def wgrad(name, shape, **kw):
    """shape = (n, h, w, c1, c2, cout, k, stride): ops.conv2d_wgrad - dw + db onto a filled buffer, then accumulated onto integers."""
    return _c('wgrad', name, shape=shape, **kw)


def wgrad_unpool(name, shape, **kw):
    """shape = (n, h, w, cin, cout): ops.conv2d_wgrad_unpool."""
    return _c('wgrad_unpool', name, shape=shape, **kw)


def epi(name, shape):
    """shape = (n, h, w, cin, cout, k): the epilogues beyond bias / activation / mask / pooling, over a bf16-stored input: LeakyReLU
    + bf16 copy at every kernel size; at 3x3 also residual + bf16 copy, the LeakyReLU copy of a plain result (copy_lrelu), the
    depth-to-space store and the space-to-depth store of an input gradient.  The 5x5 rings know none of them - the dispatch must
    step aside to the tile kernel behind them (plain_epi); the 3x3 ring ends in the tile kernel's own conv_epilogue_vec and takes
    them all."""
    return _c('epi', name, shape=shape)


def convt(name, shape, ob, **kw):
    """shape = (n, h, w, cin, cout): ops.convt2x2 over a bf16-stored input."""
    return _c('convt', name, shape=shape, ob=ob, **kw)


def cconv3(name, shape):
    return _c('cconv3', name, shape=shape)


def conv1(name, shape, ob):
    return _c('conv1', name, shape=shape, ob=ob)


POOL_ACTS = (('leaky_relu', '_lrelu'), (None, ''))
SPARSE_ENV = {'NIMG_NO_WGRAD5_SPARSE': '1'}
DGRAD5S_SHAPES = [(2, 32, 32, 32, 64), (1, 64, 64, 64, 128), (2, 16, 48, 128, 256), (2, 48, 40, 64, 64), (1, 48, 40, 192, 64)]


def _dgrad5s(tag):
    out = [dgrad_unpool('{}-{}from{}-{}x{}{}'.format(tag, s[3], s[4], s[1], s[2], '' if ob else '-f32out'), s, ob, sparse=True)
           for s in DGRAD5S_SHAPES for ob in ((True, False) if s[0] * s[1] * s[2] * s[3] <= (1 << 18) else (True,))]
    return out + [dgrad_unpool(tag + '-full', DGRAD5S_SHAPES[0], False, sparse=True, full=True)]


PLAIN = [
    fwd('plain-tn64-k3-32to64-ragged', (2, 24, 40, 32, 0, 64, 3, 1), True), fwd('plain-tn64-k3-32to64-ragged-f32out', (2, 24, 40, 32, 0, 64, 3, 1), False),
    fwd('plain-tn64-k3-16+16to64', (2, 24, 40, 16, 16, 64, 3, 1), True),
    fwd('plain-tn32-k3-16+16to48', (2, 24, 40, 16, 16, 48, 3, 1), False),
    fwd('plain-tn32-k5-32to48', (2, 24, 40, 32, 0, 48, 5, 1), False), fwd('plain-tn64-k5-32to64', (2, 32, 48, 32, 0, 64, 5, 1), True),
    fwd('plain-tn32-k5-64to32-ring32-shape', (2, 40, 72, 64, 0, 32, 5, 1), True),
    fwd('plain-8x8x4-k3-64to128', (5, 8, 8, 64, 0, 128, 3, 1), True),
    # the 32x16 tile: Cout <= 32, Hout % 32 == 0, >= 2048 tiles; Cout = 8 is the smallest ops sends to the bf16 kernels (8 MB of bf16)
    fwd('plain-32x16-k5-16to8-2048tiles', (16, 256, 256, 16, 0, 8, 5, 1), True, lrelu_only=True),
    pool('plain-tn32-pool-k5-32to64-below-384wg', (2, 32, 48, 32, 64, 5), True), pool('plain-tn32-pool-k5-32to48-f32out', (2, 24, 40, 32, 48, 5), False),
    pool('plain-tn64-pool-k5-32to128-384wg', (48, 32, 32, 32, 128, 5), True, lrelu_only=True),
    and_pool('plain-and_pool-16to64', (2, 24, 40, 16, 64)),
    epi('plain-tn64-k3-epilogues', (2, 24, 40, 32, 64, 3)), epi('plain-tn32-k5-epilogues', (2, 24, 40, 32, 48, 5)),
    dgrad('plain-dgrad-k5-32from64', (2, 32, 48, 32, 64, 5), True, mask=True), dgrad('plain-dgrad-k3-64from32', (2, 24, 40, 64, 32, 3), False, mask=True),
    dgrad_unpool('plain-unpool-materialised-32from64', (2, 32, 32, 32, 64), True, fold=False),
    dgrad_unpool('plain-unpool-materialised-64from64-f32out', (2, 16, 48, 64, 64), False, fold=False),
    fwd('plain-full-tn64-k3', (2, 24, 40, 32, 0, 64, 3, 1), True, full=True), fwd('plain-full-tn32-k5', (2, 24, 40, 32, 0, 48, 5, 1), False, full=True),
    dgrad('plain-full-dgrad-k5', (2, 32, 48, 32, 64, 5), False, full=True),
    dgrad_unpool('plain-full-unpool-materialised', (2, 32, 32, 32, 64), True, fold=False, full=True),
]

FALLBACKS = [
    fwd('buf-tn64-k3-64to64-dma-shape', (3, 16, 16, 64, 0, 64, 3, 1), True), fwd('buf-tn64-k3-64to64-dma-shape-f32out', (3, 16, 16, 64, 0, 64, 3, 1), False),
    fwd('tile-tn32-k3-16to24-ragged-dma-shape', (2, 24, 20, 16, 0, 24, 3, 1), True),
    fwd('buf-8x8x4-k3-64to128-dma4-shape', (5, 8, 8, 64, 0, 128, 3, 1), True),
    fwd('tile-tn64-k3-32+32to64-dma-shape', (2, 32, 32, 32, 32, 64, 3, 1), True),
    and_pool('buf-and_pool-64to64-dma-shape', (3, 16, 16, 64, 64)), and_pool('tile-and_pool-16to24-ragged', (2, 24, 20, 16, 24)),
    fwd('buf-tn64-k5-32to128-ring128-shape', (2, 32, 48, 32, 0, 128, 5, 1), True), fwd('buf-tn64-k5-32to128-ring128-shape-f32out', (2, 32, 48, 32, 0, 128, 5, 1), False),
    fwd('buf-tn64-k5-64to64-ring64-shape-ragged', (2, 48, 40, 64, 0, 64, 5, 1), True),
    fwd('buf-tn32-k5-64to32-ring32-shape', (2, 40, 72, 64, 0, 32, 5, 1), True),
    epi('buf-tn64-k5-epilogues-ring128-shape', (2, 32, 48, 32, 128, 5)), epi('buf-tn64-k3-epilogues-dma-shape', (3, 16, 16, 64, 64, 3)),
    pool('buf-tn32-pool-k5-32to128-below-384wg', (2, 32, 48, 32, 128, 5), True), pool('buf-tn32-pool-k5-64to64-f32out-below-384wg', (2, 48, 40, 64, 64, 5), False),
    pool('buf-tn64-pool-k5-32to128-ring128-shape-384wg', (48, 32, 32, 32, 128, 5), True, lrelu_only=True),
    dgrad('buf-dgrad-k5-64from128-ring64-shape', (2, 32, 48, 64, 128, 5), True, mask=True),
    dgrad('buf-dgrad-k5-32from64-ring32-shape', (2, 40, 72, 32, 64, 5), False, mask=True),
    dgrad_unpool('buf-unpool-tn64-64from64', (2, 32, 32, 64, 64), True), dgrad_unpool('buf-unpool-tn64-128from64-f32out', (2, 32, 32, 128, 64), False),
    dgrad_unpool('buf-unpool-tn32-32from64', (2, 32, 32, 32, 64), True),
    fwd('k1-ck16-64to64', (3, 16, 16, 64, 0, 64, 1, 1), False, xb=False), fwd('k1-ck16-64to64-bf16', (3, 16, 16, 64, 0, 64, 1, 1), True),
    fwd('k1-ck16-64+64to64', (3, 16, 16, 64, 64, 64, 1, 1), False, xb=False),
    wgrad('generic-8x8-64to128-n5', (5, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True), wgrad('generic-8x8-64to128-n4', (4, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True),
    wgrad('wide-dz-tile-k3-8to24', (2, 20, 24, 8, 0, 24, 3, 1)), wgrad('wide-dz-tile-k3-32to32-bf16', (2, 16, 24, 32, 0, 32, 3, 1), xb=True, zb=True),
    wgrad_unpool('generic-unpool-32to64', (2, 32, 32, 32, 64)), wgrad_unpool('generic-unpool-32to64-h8', (1, 8, 16, 32, 64)),
    wgrad_unpool('generic-unpool-64to192-h24', (3, 24, 32, 64, 192)),
    wgrad('c3k5-valu-w64', (2, 24, 64, 3, 0, 3, 5, 1), pad_mode=1, no_db=True), wgrad('c3k5-valu-w128-ragged', (1, 37, 128, 3, 0, 3, 5, 1), pad_mode=1, no_db=True),
    convt('convt-phases-64to32', (2, 8, 12, 64, 32), True), convt('convt-phases-24to40', (3, 16, 20, 24, 40), True),
    fwd('buf-full-tn64-k3', (3, 16, 16, 64, 0, 64, 3, 1), True, full=True), fwd('buf-full-tn64-k5', (2, 32, 48, 32, 0, 128, 5, 1), False, full=True),
    fwd('k1-ck16-full', (3, 16, 16, 64, 0, 64, 1, 1), False, xb=False, full=True),
    fwd('buf-full-tn32-k5-ring32-shape', (2, 40, 72, 64, 0, 32, 5, 1), True, full=True), convt('convt-phases-full', (2, 8, 12, 64, 32), True, full=True),
    dgrad('buf-full-dgrad-k5', (2, 32, 48, 64, 128, 5), False, full=True), dgrad_unpool('buf-full-unpool', (2, 32, 32, 64, 64), False, full=True),
]

OPTIN_A = [
    fwd('ring128nw8-32to128', (2, 32, 48, 32, 0, 128, 5, 1), True), fwd('ring128nw8-32to128-f32out', (2, 32, 48, 32, 0, 128, 5, 1), False),
    fwd('ring128nw8-64to128', (2, 32, 32, 64, 0, 128, 5, 1), True),
    fwd('ring128nw4-h48-under-nw8', (2, 48, 40, 32, 0, 128, 5, 1), True),
    pool('ring128nw8-pool-32to128-384wg', (48, 32, 32, 32, 128, 5), True, lrelu_only=True),
    dgrad('ring128nw8-dgrad-128from64', (2, 32, 48, 128, 64, 5), True, mask=True),
    dgrad_unpool('ring128nw8-unpool-128from64', (2, 32, 32, 128, 64), True),
    fwd('tile-k5-32to64-ring64-off', (2, 32, 48, 32, 0, 64, 5, 1), True), pool('tile-tn32-pool-k5-32to64-below-384wg', (2, 32, 48, 32, 64, 5), True),
    fwd('ring3-128to128', (2, 32, 48, 128, 0, 128, 3, 1), True), fwd('ring3-128to128-f32out', (2, 32, 48, 128, 0, 128, 3, 1), False),
    fwd('ring3-32to128-ragged-1600px', (2, 40, 40, 32, 0, 128, 3, 1), True),
    dgrad('ring3-dgrad-128from128', (2, 32, 48, 128, 128, 3), True, mask=True),
    epi('tile-behind-ring128nw8-k5-epilogues', (2, 32, 48, 32, 128, 5)), epi('ring3-epilogues-128to128', (2, 32, 48, 128, 128, 3)),
    fwd('dma4-pixel-major-64to128', (5, 8, 8, 64, 0, 128, 3, 1), True), fwd('dma4-pixel-major-64to128-f32out', (5, 8, 8, 64, 0, 128, 3, 1), False),
    fwd('dma4-pixel-major-6x8-64to36', (3, 6, 8, 64, 0, 36, 3, 1), True), fwd('dma4-pixel-major-32+32to64', (5, 8, 8, 32, 32, 64, 3, 1), True),
    dgrad('dma4-pixel-major-dgrad-128from64', (5, 8, 8, 128, 64, 3), True, mask=True),
    wgrad_unpool('wgrad5-8-kx3l-s1-32to64', (2, 32, 32, 32, 64), env=SPARSE_ENV), wgrad_unpool('wgrad5-8-kx3l-s1-h8', (1, 8, 16, 32, 64), env=SPARSE_ENV),
    wgrad_unpool('wgrad5-8-kx3l-s1-64to192-h24', (3, 24, 32, 64, 192), env=SPARSE_ENV),
    fwd('ring128nw8-full', (2, 32, 48, 32, 0, 128, 5, 1), False, full=True), fwd('ring3-full', (2, 32, 48, 128, 0, 128, 3, 1), True, full=True),
    fwd('dma4-pixel-major-full', (5, 8, 8, 64, 0, 128, 3, 1), True, full=True), dgrad('ring3-dgrad-full', (2, 32, 48, 128, 128, 3), True, full=True), dgrad('ring128nw8-dgrad-full', (2, 32, 48, 128, 64, 5), False, full=True),
] + _dgrad5s('sparse16')

OPTIN_B = [
    fwd('ring64-at-128-channels', (2, 32, 48, 32, 0, 128, 5, 1), True), fwd('ring64-at-128-channels-f32out', (2, 32, 48, 32, 0, 128, 5, 1), False),
    fwd('ring128-h24-under-tn64', (2, 24, 40, 32, 0, 128, 5, 1), True),
    pool('ring64-pool-at-128-channels-384wg', (48, 32, 32, 32, 128, 5), True, lrelu_only=True), dgrad('ring64-dgrad-128from64', (2, 32, 48, 128, 64, 5), True, mask=True),
    dgrad_unpool('ring64-unpool-128from64', (2, 32, 32, 128, 64), True), epi('tile-behind-ring64-k5-epilogues', (2, 32, 48, 32, 128, 5)),
    fwd('buf-tn32-k5-64to32-ring32-off', (2, 40, 72, 64, 0, 32, 5, 1), True), dgrad('buf-tn32-dgrad-32from64-ring32-off', (2, 40, 72, 32, 64, 5), False, mask=True),
    dgrad_unpool('buf-tn32-unpool-32from64-ring32-off', (2, 32, 32, 32, 64), True),
    wgrad_unpool('wgrad5-16-kx3l-s1-32to64', (2, 32, 32, 32, 64), env=SPARSE_ENV), wgrad_unpool('wgrad5-16-kx3l-s1-64to128', (1, 16, 32, 64, 128), env=SPARSE_ENV),
    wgrad('c3k5-mfma16-w64', (2, 24, 64, 3, 0, 3, 5, 1), pad_mode=1, no_db=True), wgrad('c3k5-mfma16-w128-ragged', (1, 37, 128, 3, 0, 3, 5, 1), pad_mode=1, no_db=True),
    fwd('rows-ncw4-pfd1-32to32', (2, 20, 128, 32, 0, 32, 3, 1), True, rows=True), fwd('rows-ncw4-pfd1-32to32-f32out-h128', (1, 128, 128, 32, 0, 32, 3, 1), False, rows=True),
    dgrad('rows-ncw4-pfd1-dgrad-32from32', (2, 20, 128, 32, 32, 3), True, mask=True, rows=True), and_pool('rows-ncw4-pfd1-and_pool-32to32', (2, 20, 128, 32, 32), rows=True),
    cconv3('cconv-64x1-w128-ragged', (1, 37, 128)), cconv3('cconv-64x1-w320', (2, 10, 320)), cconv3('cconv-16x1-w64', (2, 24, 64)),
    fwd('ring64-at-128-channels-full', (2, 32, 48, 32, 0, 128, 5, 1), False, full=True),
    fwd('buf-tn32-ring32-off-full', (2, 40, 72, 64, 0, 32, 5, 1), True, full=True), dgrad('buf-tn32-dgrad-ring32-off-full', (2, 40, 72, 32, 64, 5), False, full=True),
] + _dgrad5s('sparse-block42')

W5 = [{}, {'NIMG_WGRAD5_W4': '1'}, SPARSE_ENV]
SPLITS = [
    # (the targets bind where the default 256 / blocks_io is below both the work and the workspace bound 512 / blocks_io)
    wgrad('alltaps3-maxslabs-64to64-144slabs', (3, 48, 128, 64, 0, 64, 3, 1), xb=True, zb=True, plan=(2, 8, 144), plan_default=(2, 8, 72)),
    wgrad('alltaps3-maxslabs-128to64-68slabs-ragged', (3, 72, 80, 128, 0, 64, 3, 1), xb=True, zb=True, plan=(2, 8, 68), plan_default=(2, 8, 45)),
    wgrad('alltaps3-maxslabs-32to32', (3, 32, 32, 32, 0, 32, 3, 1), xb=True, zb=True, plan=(1, 16, 12), plan_default=(1, 16, 12)),
    wgrad('generic-k5-512blocks-32to128-135slabs', (3, 80, 144, 32, 0, 128, 5, 1), xb=True, zb=True, slabs=135, slabs_default=68),
    wgrad('generic-k5-512blocks-f32', (5, 32, 32, 32, 0, 64, 5, 1), slabs=20, slabs_default=20),
] + [wgrad_unpool('wgrad5-maxslabs-32to64-{}'.format(i), (2, 32, 32, 32, 64), env=e) for i, e in enumerate(W5)] + [
    wgrad_unpool('wgrad5-maxslabs-64to128-80slabs-{}'.format(i), (5, 64, 64, 64, 128), env=e) for i, e in enumerate(W5)] + [
    wgrad_unpool('wgrad5-maxslabs-64to192-h72-54slabs', (3, 72, 64, 64, 192))] + [
    fwd('rows-3wgs-bh4-ncw4-32to32', (2, 20, 128, 32, 0, 32, 3, 1), True, rows=True), fwd('rows-3wgs-bh4-ncw4-32to32-f32out', (2, 20, 128, 32, 0, 32, 3, 1), False, rows=True),
    fwd('rows-3wgs-bh4-64to32', (2, 20, 128, 64, 0, 32, 3, 1), True, rows=True), fwd('rows-3wgs-bh4-32+32to32', (3, 12, 128, 32, 32, 32, 3, 1), True, rows=True),
    dgrad('rows-3wgs-bh4-dgrad-32from32', (2, 20, 128, 32, 32, 3), True, mask=True, rows=True),
    dgrad('rows-3wgs-bh4-dgrad-64from32-two-outputs', (2, 20, 128, 64, 32, 3), True, split=True, rows=True),
    and_pool('rows-3wgs-bh4-and_pool-32to32', (2, 20, 128, 32, 32), rows=True),
    fwd('rows-full', (2, 20, 128, 32, 0, 32, 3, 1), True, rows=True, full=True), dgrad('rows-dgrad-full', (2, 20, 128, 32, 32, 3), True, rows=True, full=True),
    cconv3('cconv-cap256-260tiles', (2, 1040, 68)), conv1('conv1-cap256-264tiles', (2, 528, 68), True),
    fwd('buf-k3-64to64-dma-maxhw0', (3, 16, 16, 64, 0, 64, 3, 1), True), fwd('dma-32+32to64-dma-maxhw0', (2, 16, 16, 32, 32, 64, 3, 1), True),
]

# ---- the ticket finish.  `slabs`: what the restatement above must give (asserted by the CPU self-test; the grids of the kernel trace
# are blocks_io * slabs).  24 / 25: the last one-level and the first two-level count; 27: groups of 6, 6, 6, 6, 3.
NB = lambda v: {'NIMG_WGRAD3_NB': str(v)}
TICKETS = [
    wgrad('tk-generic-k3-24to40-1slab', (1, 8, 16, 24, 0, 40, 3, 1), slabs=1), wgrad('tk-generic-k3-24to40-2slabs', (2, 8, 16, 24, 0, 40, 3, 1), slabs=2),
    wgrad('tk-generic-k3-24to40-24slabs', (2, 24, 64, 24, 0, 40, 3, 1), slabs=24), wgrad('tk-generic-k3-24to40-25slabs', (1, 40, 80, 24, 0, 40, 3, 1), slabs=25),
    wgrad('tk-generic-k3-24to40-27slabs', (3, 24, 48, 24, 0, 40, 3, 1), slabs=27),
    wgrad('tk-generic-k3-8to4-smallest-cout', (2, 16, 24, 8, 0, 4, 3, 1), slabs=8), wgrad('tk-generic-k3-40to72-two-tiles', (3, 16, 16, 40, 0, 72, 3, 1), slabs=6),
    wgrad('tk-generic-k3-16+16to36', (2, 16, 24, 16, 16, 36, 3, 1), slabs=8),
    wgrad('tk-generic-k3-bf16-x-only', (3, 16, 24, 32, 0, 64, 3, 1), xb=True, slabs=12), wgrad('tk-generic-k3-bf16-both-w24', (3, 16, 24, 32, 0, 40, 3, 1), xb=True, zb=True, slabs=12),
    wgrad('tk-generic-k1-48to32', (5, 16, 20, 48, 0, 32, 1, 1), xb=True, zb=True, slabs=20), wgrad('tk-generic-k1-64to64-f32', (3, 16, 16, 64, 0, 64, 1, 1), slabs=6),
    wgrad('tk-generic-k5-40to72-ragged', (1, 37, 19, 40, 0, 72, 5, 1), slabs=6), wgrad('tk-generic-k5-32to64-bf16', (3, 24, 40, 32, 0, 64, 5, 1), xb=True, zb=True, slabs=18),
    wgrad('tk-generic-s2-k5-16to32', (2, 32, 32, 16, 0, 32, 5, 2), slabs=4), wgrad('tk-generic-k2-s2-24to40', (2, 16, 24, 24, 0, 40, 2, 2), slabs=2),
    wgrad('tk-generic-k2-s2-bf16', (2, 16, 32, 32, 0, 64, 2, 2), xb=True, zb=True, slabs=2),
    wgrad('tk-pair8-64to128-n5', (5, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True, slabs=3), wgrad('tk-pair8-64to128-n4', (4, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True, slabs=2),
    wgrad('tk-pair8-128to192-n5', (5, 8, 8, 128, 0, 192, 3, 1), xb=True, zb=True, slabs=3),
    wgrad('tk-alltaps3-nb1-th16-32to32', (2, 16, 32, 32, 0, 32, 3, 1), xb=True, zb=True, slabs=4),
    wgrad('tk-alltaps3-nb1-th8-25slabs', (1, 40, 80, 32, 0, 32, 3, 1), xb=True, zb=True, slabs=25),
    wgrad('tk-alltaps3-nb1-th8-27slabs', (3, 24, 48, 32, 0, 32, 3, 1), xb=True, zb=True, slabs=27),
    wgrad('tk-alltaps3-nb2-32+32to64', (2, 16, 32, 32, 32, 64, 3, 1), xb=True, zb=True, slabs=8),
    wgrad('tk-alltaps3-nb4-64to128', (3, 16, 32, 64, 0, 128, 3, 1), xb=True, zb=True, slabs=12),
    wgrad('tk-alltaps3-nb1-forced-64to128', (3, 16, 32, 64, 0, 128, 3, 1), xb=True, zb=True, env=NB(1), slabs=6),
    wgrad('tk-alltaps3-nb2-forced-64+64to128', (2, 24, 32, 64, 64, 128, 3, 1), xb=True, zb=True, env=NB(2), slabs=12),
    wgrad('tk-no-db', (2, 24, 64, 24, 0, 40, 3, 1), no_db=True, slabs=24), wgrad('tk-alltaps3-no-db', (2, 16, 32, 32, 0, 32, 3, 1), xb=True, zb=True, no_db=True, slabs=4),
    wgrad('tk-misaligned-dw-falls-back', (2, 24, 64, 24, 0, 40, 3, 1), misaligned=True, slabs=24),
    wgrad('tk-alltaps3-misaligned-dw-falls-back', (2, 16, 32, 32, 0, 32, 3, 1), xb=True, zb=True, misaligned=True, slabs=4),
    wgrad('tk-small-binding-falls-back', (1, 40, 80, 24, 0, 40, 3, 1), small_binding=True, slabs=25),
    wgrad('tk-side-streams', (3, 24, 48, 24, 0, 40, 3, 1), side=True, slabs=27),
    wgrad('tk-alltaps3-side-streams', (1, 40, 80, 32, 0, 32, 3, 1), xb=True, zb=True, side=True, slabs=25),
    wgrad('tk-full-generic', (3, 24, 48, 24, 0, 40, 3, 1), full=True, slabs=27), wgrad('tk-full-alltaps3', (1, 40, 80, 32, 0, 32, 3, 1), xb=True, zb=True, full=True, slabs=25),
    wgrad('tk-full-pair8', (5, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True, full=True, slabs=3),
]
TICKETS_SPLITS = [
    wgrad('tks-alltaps3-64to64-144slabs', (3, 48, 128, 64, 0, 64, 3, 1), xb=True, zb=True, slabs=144),                  # 12 groups of 12
    wgrad('tks-alltaps3-128to64-68slabs-ragged', (3, 72, 80, 128, 0, 64, 3, 1), xb=True, zb=True, slabs=68),           # 9, ..., 9, 5; last split 1 tile
    wgrad('tks-alltaps3-nb1-forced-64to64-72slabs', (3, 24, 128, 64, 0, 64, 3, 1), xb=True, zb=True, env=NB(1), slabs=72),
    wgrad('tks-alltaps3-64+64to192', (2, 32, 32, 64, 64, 192, 3, 1), xb=True, zb=True, slabs=16),
    wgrad('tks-generic-k3-48to96', (3, 16, 16, 48, 0, 96, 3, 1), slabs=6),
    wgrad('tks-full-alltaps3', (3, 48, 128, 64, 0, 64, 3, 1), xb=True, zb=True, full=True, slabs=144),
]

NO_TICKETS = [
    wgrad('ntk-generic-k3-24to40-25slabs', (1, 40, 80, 24, 0, 40, 3, 1), slabs=25), wgrad('ntk-alltaps3-nb1-th8-27slabs', (3, 24, 48, 32, 0, 32, 3, 1), xb=True, zb=True, slabs=27),
    wgrad('ntk-pair8-64to128-n5', (5, 8, 8, 64, 0, 128, 3, 1), xb=True, zb=True, slabs=3), wgrad('ntk-side-streams', (3, 24, 48, 24, 0, 40, 3, 1), side=True, slabs=27),
    wgrad('ntk-full-generic', (3, 24, 48, 24, 0, 40, 3, 1), full=True, slabs=27), wgrad('ntk-full-alltaps3', (1, 40, 80, 32, 0, 32, 3, 1), xb=True, zb=True, full=True, slabs=25),
    wgrad_unpool('wgrad5-16-kx3l-s2-32to64', (2, 32, 32, 32, 64), env=SPARSE_ENV), wgrad_unpool('wgrad5-8-kx3l-s2-64to192-h24', (3, 24, 32, 64, 192), env=SPARSE_ENV),
    wgrad_unpool('wgrad5-8-kx3l-s2-h8', (1, 8, 16, 32, 64), env=SPARSE_ENV),
]

GROUPS = {
    'plain': dict(env={'NIMG_NO_BUFFER_LOADS': '1', 'NIMG_TN32_BELOW': '0'}, cases=PLAIN),
    'fallbacks': dict(env={'NIMG_NO_CONV3_DMA': '1', 'NIMG_NO_CONV5_RING': '1', 'NIMG_NO_CK64': '1', 'NIMG_NO_CONVT_FAT': '1',
                           'NIMG_NO_WGRAD_PAIR8': '1', 'NIMG_NO_NARROW_WGRAD': '1', 'NIMG_NO_WGRAD5_ALLTAPS': '1', 'NIMG_NO_C3K5_MFMA': '1',
                           'NIMG_TN32_BELOW': '0'}, cases=FALLBACKS),
    'optin_a': dict(env={'NIMG_RING_NW8': '1', 'NIMG_CONV3_RING_MIN': '0', 'NIMG_NO_CONV5_RING64': '1', 'NIMG_DGRAD5S_ACC16': '1',
                         'NIMG_CONV3_PLANES': '0', 'NIMG_WGRAD5_TH8': '1', 'NIMG_WGRAD5_KX3L': '1', 'NIMG_WGRAD5_SCHED': '1',
                         'NIMG_TN32_BELOW': '0'}, cases=OPTIN_A),
    'optin_b': dict(env={'NIMG_DGRAD5S_BLOCK42': '1', 'NIMG_RING_TN64': '1', 'NIMG_NO_CONV5_RING32': '1', 'NIMG_WGRAD5_KX3L': '1',
                         'NIMG_WGRAD5_SCHED': '1', 'NIMG_C3K5_TR8': '0', 'NIMG_CCONV_VARIANT': '1', 'NIMG_ROWS_NCW': '4', 'NIMG_ROWS_PFD': '1',
                         'NIMG_TN32_BELOW': '0'}, cases=OPTIN_B),
    'splits': dict(env={'NIMG_WGRAD3_BLOCKS': BIG, 'NIMG_WGRAD5_BLOCKS': '512', 'NIMG_WGRAD5_ALLTAPS_BLOCKS': BIG, 'NIMG_ROWS_WGS': '3',
                        'NIMG_ROWS_BH': '4', 'NIMG_ROWS_NCW': '4', 'NIMG_WGRAD5_SCHED': '1', 'NIMG_CCONV_CAP': '1', 'NIMG_CONV1_CAP': '1',
                        'NIMG_CONV3_DMA_MAXHW': '0'}, cases=SPLITS),
    'tickets': dict(env={'NIMG_TICKETS': '1'}, cases=TICKETS),
    'tickets_splits': dict(env={'NIMG_TICKETS': '1', 'NIMG_WGRAD3_BLOCKS': BIG, 'NIMG_TN32_BELOW': '0'}, cases=TICKETS_SPLITS),
    # the library-side veto: streams are bound as in 'tickets', every launch must take the slabs + reduction launch all the same
    'no_tickets': dict(env={'NIMG_TICKETS': '1', 'NIMG_NO_TICKETS': '1', 'NIMG_WGRAD5_KX3L': '1'}, cases=NO_TICKETS),
}
TICKET_GROUPS = ('tickets', 'tickets_splits', 'no_tickets')

# per-call switches, run inside the pytest process (section 4 of the module header)
PER_CALL_CASES = [
    wgrad('generic-at-alltaps3-32to32-128px', (1, 64, 128, 32, 0, 32, 3, 1), xb=True, zb=True, env={'NIMG_NO_WGRAD3_ALLTAPS': '1'}),
    wgrad('generic-at-alltaps3-32+32to32', (2, 32, 64, 32, 32, 32, 3, 1), xb=True, zb=True, env={'NIMG_NO_WGRAD3_ALLTAPS': '1'}),
    wgrad('generic-at-alltaps3-128+128to128', (3, 16, 32, 128, 128, 128, 3, 1), xb=True, zb=True, env={'NIMG_NO_WGRAD3_ALLTAPS': '1'}),
    wgrad('generic-at-alltaps3-ragged-64to32', (2, 24, 32, 64, 0, 32, 3, 1), xb=True, zb=True, env={'NIMG_NO_WGRAD3_ALLTAPS': '1'}),
    wgrad('alltaps3-nb1-th16-at-128-channels', (3, 32, 32, 64, 0, 128, 3, 1), xb=True, zb=True, env=NB(1)),
    wgrad('alltaps3-nb1-th8-at-128-channels', (3, 24, 32, 64, 0, 128, 3, 1), xb=True, zb=True, env=NB(1)),
    wgrad('alltaps3-nb2-th8-at-128-channels-h32', (3, 32, 32, 64, 0, 128, 3, 1), xb=True, zb=True, env=NB(2)),
    wgrad('alltaps3-nb2-th8-at-128-channels-h24', (3, 24, 32, 32, 32, 128, 3, 1), xb=True, zb=True, env=NB(2)),
]
REDUCE_STREAM_CASES = [
    wgrad('rstream-generic-k3-24to40', (3, 24, 48, 24, 0, 40, 3, 1), side=True), wgrad('rstream-alltaps3-32to32', (1, 40, 80, 32, 0, 32, 3, 1), xb=True, zb=True, side=True),
    wgrad('rstream-generic-k5-32to64', (3, 24, 40, 32, 0, 64, 5, 1), xb=True, zb=True, side=True),
]


def all_cases():
    for g in GROUPS.values():
        for c in g['cases']:
            yield c
    for c in PER_CALL_CASES + REDUCE_STREAM_CASES:
        yield c


# ----------------------------------------------------------------------------------------------------------------------
# operands and references
def full_mantissa(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def _gens(case, stores_bf16):
    """(generator of pixels, generator of weights): integers that stay exact, or full-mantissa values on the bf16 grid."""
    if case.get('full'):
        return (lambda s, seed, *a: bf16_rne(full_mantissa(s, seed)).astype(np.float32),
                lambda s, seed, *a: bf16_rne(0.2 * full_mantissa(s, seed)).astype(np.float32))
    g = ternary if stores_bf16 else small_ints
    return g, g


def conv_ref(x, wt, b, stride=1, padding='SAME', pad_mode=0):
    def one(x_, w_, b_):
        xt, pd = to64(x_), padding
        if pad_mode:
            xt, pd = T.pad2d(xt, (w_.shape[0] - 1) // 2, PAD_NAMES[pad_mode]), 'VALID'
        return T.conv2d(xt, to64(w_), None if b_ is None else to64(b_), stride, pd).numpy()
    return one(x, wt, b), one(np.abs(x), np.abs(wt), None if b is None else np.abs(b))


def flipped(wt):
    return np.ascontiguousarray(wt[::-1, ::-1].transpose(0, 1, 3, 2))


def wgrad_ref(x, dz, k, stride, pad_mode=0, padding='SAME'):
    def one(x_, dz_):
        wt = torch.zeros((k, k, x_.shape[3], dz_.shape[3]), dtype=torch.float64, requires_grad=True)
        xt = to64(x_)
        if pad_mode:
            z = T.conv2d(T.pad2d(xt, (k - 1) // 2, PAD_NAMES[pad_mode]), wt, None, stride, 'VALID')
        else:
            z = T.conv2d(xt, wt, None, stride, padding)
        assert tuple(z.shape) == tuple(dz_.shape), (z.shape, dz_.shape)
        (z * to64(dz_)).sum().backward()
        return wt.grad.numpy()
    return one(x, dz), one(np.abs(x), np.abs(dz))


def planted_idx(shape, seed):
    return np.random.default_rng(seed).integers(0, 4, size=shape).astype(np.uint8)


def _conditions(case, absum, ref, stores_bf16, what=''):
    if not case.get('full'):
        assert_exact_conditions(absum, ref, stores_bf16, what=case['name'] + ' ' + what)


def finish(ref, act, stores_bf16):
    """What a kernel must store: the exact value, LeakyReLU as one float32 multiply, one rounding where the output is bf16."""
    want = ref if act is None else lrelu_f32(ref)
    return bf16_rne(want) if (stores_bf16 and act is not None) else np.asarray(want, np.float64)


@functools.lru_cache(maxsize=None)
def _operands_cached(name):
    return _operands(BY_NAME[name])


def operands(case):
    return _operands_cached(case['name'])


def _operands(case):
    kind, ob = case['kind'], case.get('ob', False)
    gx, gw = _gens(case, ob)
    if kind == 'fwd':
        n, h, w, c1, c2, cout, k, s = case['shape']
        return dict(x=gx((n, h, w, c1 + c2), 1), w=gw((k, k, c1 + c2, cout), 2), b=gx((cout,), 3))
    if kind == 'dgrad':
        n, h, w, cin, cout, k = case['shape']
        return dict(dz=gx((n, h, w, cout), 4), w=gw((k, k, cin, cout), 5), m=small_ints((n, h, w, cin), 6, 1))
    if kind == 'pool':
        n, h, w, cin, cout, k = case['shape']
        return dict(x=gx((n, h, w, cin), 11), w=gw((k, k, cin, cout), 12), b=gx((cout,), 13))
    if kind == 'and_pool':
        n, h, w, cin, cout = case['shape']
        return dict(x=ternary((n, h, w, cin), 14), w=ternary((3, 3, cin, cout), 15), b=ternary((cout,), 16))
    if kind == 'dgrad_unpool':
        n, h, w, cin, cout = case['shape']
        return dict(gp=gx((n, h // 2, w // 2, cout), 17), w=gw((5, 5, cin, cout), 18), idx=planted_idx((n, h // 2, w // 2, cout), 19),
                    m=small_ints((n, h, w, cin), 20, 1))
    if kind == 'wgrad':
        n, h, w, c1, c2, cout, k, s = case['shape']
        gx, _ = _gens(case, False)
        return dict(x=gx((n, h, w, c1 + c2), 7), dz=gx((n, cdiv(h, s), cdiv(w, s), cout), 8), dw0=small_ints((k, k, c1 + c2, cout), 9, 100),
                    db0=small_ints((cout,), 10, 100))
    if kind == 'wgrad_unpool':
        n, h, w, cin, cout = case['shape']
        return dict(x=small_ints((n, h, w, cin), 21), gp=small_ints((n, h // 2, w // 2, cout), 22), idx=planted_idx((n, h // 2, w // 2, cout), 23))
    if kind == 'epi':
        n, h, w, cin, cout, k = case['shape']
        return dict(x=small_ints((n, h, w, cin), 31), r=small_ints((n, h, w, cout), 32), w=small_ints((k, k, cin, cout), 33), b=small_ints((cout,), 34),
                    w2=small_ints((k, k, cout, cin), 35))          # (w2: the kernel whose input gradient, taken of x, has cout channels)
    if kind == 'convt':
        n, h, w, cin, cout = case['shape']
        return dict(x=gx((n, h, w, cin), 51), w=gw((2, 2, cout, cin), 52), b=gx((cout,), 53))
    if kind == 'cconv3':
        n, h, w = case['shape']
        return dict(x=ternary((n, h, w, 3), 61, 0.5), w=small_ints((5, 5, 3, 3), 62))
    if kind == 'conv1':
        n, h, w = case['shape']
        return dict(x=gx((n, h, w, 3), 64), w=gw((5, 5, 3, 32), 65), b=gx((32,), 66))
    raise KeyError(kind)


_POOL_REFS = {}


@functools.lru_cache(maxsize=None)
def _reference_cached(name):
    return _reference(BY_NAME[name])


def reference(case):
    """{key: array} - what the child must store under case['name'] + '/' + key (float64 values, uint8 arg-max bytes)."""
    return _reference_cached(case['name'])


def _reference(case):
    kind, ob, full = case['kind'], case.get('ob', False), bool(case.get('full'))
    o = operands(case)
    if kind == 'fwd':
        k, s = case['shape'][6:]
        ref, absum = conv_ref(o['x'], o['w'], o['b'], s)
        _conditions(case, absum, ref, ob)
        if case.get('lrelu_only'):
            return {'y_lrelu': finish(ref, 'leaky_relu', ob)}
        return {'y': ref} if full else {'y': finish(ref, None, ob), 'y_lrelu': finish(ref, 'leaky_relu', ob)}
    if kind == 'dgrad':
        ref, absum = conv_ref(o['dz'], flipped(o['w']), None)
        _conditions(case, absum, ref, ob)
        if full or case.get('split'):
            return {'dx': ref}
        want = mask_f32(ref, o['m'])
        return {'dx': ref, 'dx_mask': bf16_rne(want) if ob else want}
    if kind == 'pool':
        key = (case['shape'], ob)                       # (the 384-workgroup cases of four groups share one convolution)
        if key not in _POOL_REFS:
            _POOL_REFS[key] = conv_ref(o['x'], o['w'], o['b'])
        ref, absum = _POOL_REFS[key]
        _conditions(case, absum, ref, ob)
        out = {}
        for act, tag in POOL_ACTS[:1 if case.get('lrelu_only') else 2]:
            fullres = ref if act is None else lrelu_f32(ref).astype(np.float64)
            want, idx = first_max_pool(fullres)
            assert (idx != first_max_pool(fullres, last=True)[1]).any(), 'the case has no ties'
            out['pooled' + tag], out['idx' + tag] = (bf16_rne(want) if (ob and act) else want), idx
        return out
    if kind == 'and_pool':
        ref, absum = conv_ref(o['x'], o['w'], o['b'])
        _conditions(case, absum, ref, True)
        out = {}
        for act, tag in (('leaky_relu', '_lrelu'), (None, '')):
            want = finish(ref, act, True)
            out['y' + tag], out['pooled' + tag] = want, first_max_pool(want)[0]
        return out
    if kind == 'dgrad_unpool':
        ref, absum = conv_ref(unpool(o['gp'], o['idx']), flipped(o['w']), None)
        _conditions(case, absum, ref, ob)
        fold = np.uint8([1 if case['fold'] else 0])
        if full:
            return {'dx': ref, 'fold_ok': fold}
        want = mask_f32(ref, o['m'])
        return {'dx': ref, 'dx_mask': bf16_rne(want) if ob else want, 'fold_ok': fold}
    if kind == 'wgrad':
        k, s = case['shape'][6:]
        pad_mode = case.get('pad_mode', 0)
        ref, absum = wgrad_ref(o['x'], o['dz'], k, s, pad_mode)
        dbr = o['dz'].astype(np.float64).sum(axis=(0, 1, 2))
        _conditions(case, absum + 100.0, ref, False)
        _conditions(case, np.abs(o['dz']).sum(axis=(0, 1, 2)) + 100.0, dbr, False, 'bias')
        out = {'dw': ref, 'dw_again': ref}
        if not case.get('no_db'):
            out.update(db=dbr, db_again=dbr)
        if not full:
            out['dw_acc'] = ref + o['dw0']
            if not case.get('no_db'):
                out['db_acc'] = dbr + o['db0']
        return out
    if kind == 'wgrad_unpool':
        dz = unpool(o['gp'], o['idx'])
        ref, absum = wgrad_ref(o['x'], dz, 5, 1)
        _conditions(case, absum, ref, False)
        return {'dw': ref, 'db': dz.astype(np.float64).sum(axis=(0, 1, 2))}
    if kind == 'epi':
        ref, absum = conv_ref(o['x'], o['w'], o['b'])
        _conditions(case, absum + 3.0, ref + o['r'], False)
        out = {'y_copy': lrelu_f32(ref).astype(np.float64), 'cp_copy': bf16_rne(lrelu_f32(ref))}
        if case['shape'][5] == 3:
            out.update(y_res=ref + o['r'], cp_res=bf16_rne(ref + o['r']), y_plain=ref, cp_lrelu=bf16_rne(lrelu_f32(ref)),
                       y_d2s=T.depth_to_space(to64(ref), 2).numpy())
            dref, dabs = conv_ref(o['x'], flipped(o['w2']), None)
            _conditions(case, dabs, dref, False, 'input gradient')
            out['dx_s2d'] = T.space_to_depth(to64(dref), 2).numpy()
        return out
    if kind == 'convt':
        ref = T.conv2d_transpose_2x2(to64(o['x']), to64(o['w']), to64(o['b'])).numpy()
        absum = T.conv2d_transpose_2x2(to64(np.abs(o['x'])), to64(np.abs(o['w'])), to64(np.abs(o['b']))).numpy()
        _conditions(case, absum, ref, ob)
        return {'y': ref}
    if kind == 'cconv3':
        ref, absum = conv_ref(o['x'], o['w'], None, pad_mode=1)
        _conditions(case, absum, ref, True)
        return {'y': ref, 'c4': np.concatenate([ref, np.ones(ref.shape[:3] + (1,))], axis=-1)}
    if kind == 'conv1':
        ref, absum = conv_ref(o['x'], o['w'], o['b'])
        _conditions(case, absum, ref, ob)
        out = {}
        for act, tag in (('leaky_relu', '_lrelu'), (None, '')):
            fullres = ref if act is None else lrelu_f32(ref).astype(np.float64)
            want, idx = first_max_pool(fullres)
            out['pooled' + tag], out['idx' + tag] = (bf16_rne(want) if (ob and act) else want), pack_argmax2(idx)
        return out
    raise KeyError(kind)


def pack_argmax2(idx):
    """(n, h, w, 32) arg-max codes 0..3 -> (n, h, w, 8) bytes: channel c in byte c >> 2 at bits 2 (c & 3) (include/nimg.h)."""
    i = idx.astype(np.uint8).reshape(idx.shape[:3] + (idx.shape[3] // 4, 4))
    return (i[..., 0] | (i[..., 1] << 2) | (i[..., 2] << 4) | (i[..., 3] << 6)).astype(np.uint8)


def stores_bf16(case, key):
    """Is result `key` of the case stored as bf16 by the kernel (the tolerance of a full-mantissa case depends on it)?"""
    return bool(case.get('ob')) and case['kind'] in ('fwd', 'dgrad', 'dgrad_unpool', 'convt')


def check_full(name, got, ref, bf16_out):
    """The tolerances of test_gpu_exact.check_full_mantissa: float32 outputs max|got - ref| <= 2e-5 max|ref|, bf16 outputs
    |got - ref| <= 2^-8 |ref| + 2e-5 max|ref| per element.  Returns the worst ratio (<= 1 passes)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = np.abs(ref).max()
    d = np.abs(got - ref)
    worst = float((d / (2.0 ** -8 * np.abs(ref) + 2e-5 * scale)).max()) if bf16_out else float(d.max() / scale / 2e-5)
    assert worst <= 1.0, 'full mantissa {}: error / tolerance = {:.3f}'.format(name, worst)
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# the GPU half: one case -> ([(key, tensor)], description of the ops calls made)
class per_call_env(object):
    """The switches csrc/ reads on every call, set around one call (the pytest process uses monkeypatch for the same)."""

    def __init__(self, env):
        self.env, self.old = dict(env or {}), {}

    def __enter__(self):
        for k, v in self.env.items():
            assert k in PER_CALL, k
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        return False


def run(case, ops, dev):
    """One case on the GPU -> ([(key, tensor)], the ops calls made).  ops.ROWS_CONV / ops.SPARSE_DGRAD are set as the case says and
    put back afterwards."""
    saved = ops.ROWS_CONV, ops.SPARSE_DGRAD
    try:
        if 'rows' in case:
            ops.ROWS_CONV = bool(case['rows'])
        return _run(case, ops, dev)
    finally:
        ops.ROWS_CONV, ops.SPARSE_DGRAD = saved


def _run(case, ops, dev):
    BF = torch.bfloat16

    def dv(a, bf=False):
        t = torch.from_numpy(np.array(a, dtype=np.float32, order='C')).to(dev).contiguous()
        return t.to(BF) if bf else t

    kind, ob = case['kind'], case.get('ob', False)
    o = operands(case)
    ops.set_compute('bf16')
    out = []
    if kind == 'fwd':
        n, h, w, c1, c2, cout, k, s = case['shape']
        xb = case.get('xb', False)
        x1, x2 = dv(o['x'][..., :c1], xb), (dv(o['x'][..., c1:], xb) if c2 else None)
        if case.get('rows'):
            probe = torch.empty((n, h, w, cout), dtype=BF if ob else torch.float32, device=dev)
            assert ops.rows_conv_ok(x1, x2, k, s, cout, (h, w), (1, 1), 0, probe, None, None, None), 'not a rows shape'
        for act, tag in ((None, ''),) if case.get('full') else (('leaky_relu', '_lrelu'),) if case.get('lrelu_only') else ((None, ''), ('leaky_relu', '_lrelu')):
            out.append(('y' + tag, ops.conv2d(x1, dv(o['w']), dv(o['b']), x2=x2, stride=s, act=act, out_bf16=ob)))
        what = 'ops.conv2d(x{} {}, k {}, stride {}, act None / leaky_relu, out_bf16={})'.format(' + x2' if c2 else '', 'bf16' if xb else 'f32', k, s, ob)
    elif kind == 'dgrad':
        n, h, w, cin, cout, k = case['shape']
        dzd, wd = dv(o['dz'], case.get('zb', False)), dv(o['w'])
        if case.get('split'):
            o1, o2 = (torch.empty((n, h, w, cin // 2), dtype=BF if ob else torch.float32, device=dev) for _ in range(2))
            ops.conv2d_dgrad(dzd, wd, (h, w), out=o1, out2=o2)
            out.append(('dx', torch.cat([o1, o2], dim=-1)))
        else:
            out.append(('dx', ops.conv2d_dgrad(dzd, wd, (h, w), out_bf16=ob)))
            if not case.get('full'):
                out.append(('dx_mask', ops.conv2d_dgrad(dzd, wd, (h, w), act_mask=dv(o['m'], case.get('zb', False)), out_bf16=ob)))
        what = 'ops.conv2d_dgrad(dz {}, k {}, out_bf16={}{})'.format('bf16' if case.get('zb') else 'f32', k, ob, ', out2' if case.get('split') else ', act_mask')
    elif kind == 'pool':
        xd = dv(o['x'], True)
        for act, tag in POOL_ACTS[:1 if case.get('lrelu_only') else 2]:
            pooled, idx = ops.conv2d_pool(xd, dv(o['w']), dv(o['b']), act=act, out_bf16=ob)
            out += [('pooled' + tag, pooled), ('idx' + tag, idx)]
        what = 'ops.conv2d_pool(x bf16, k {}, out_bf16={})'.format(case['shape'][5], ob)
    elif kind == 'and_pool':
        xd = dv(o['x'], True)
        assert ops.conv2d_and_pool_ok(xd, dv(o['w']))
        for act, tag in (('leaky_relu', '_lrelu'), (None, '')):
            y, pooled = ops.conv2d_and_pool(xd, dv(o['w']), dv(o['b']), act=act)
            out += [('y' + tag, y), ('pooled' + tag, pooled)]
        what = 'ops.conv2d_and_pool(x bf16)'
    elif kind == 'dgrad_unpool':
        n, h, w, cin, cout = case['shape']
        ops.SPARSE_DGRAD = bool(case['sparse'])
        gd, idd, wd = dv(o['gp'], True), torch.from_numpy(o['idx']).to(dev), dv(o['w'])
        ok = ops.unpool_fold_ok(torch.empty((n, h, w, cin), dtype=BF, device=dev), gd, cin, cout, 5)
        out.append(('fold_ok', torch.tensor([1 if ok else 0], dtype=torch.uint8)))
        masks = (None,) if case.get('full') else (None, dv(o['m'], True))
        for m, tag in zip(masks, ('dx', 'dx_mask')):
            if case['fold']:
                out.append((tag, ops.conv2d_dgrad_unpool(gd, idd, wd, act_mask=m, out_bf16=ob)))
            else:
                dz = ops.maxpool2_unpool(gd, idd, None, apply_mask=False, out_bf16=True)
                out.append((tag, ops.conv2d_dgrad(dz, wd, (h, w), act_mask=m, out_bf16=ob)))
        what = ('ops.conv2d_dgrad_unpool(SPARSE_DGRAD={}, out_bf16={})'.format(case['sparse'], ob) if case['fold'] else
                'ops.maxpool2_unpool + ops.conv2d_dgrad(out_bf16={})'.format(ob))
    elif kind == 'wgrad':
        out, what = _run_wgrad(case, ops, dev, dv, o)
    elif kind == 'wgrad_unpool':
        n, h, w, cin, cout = case['shape']
        xd, gd, idd = dv(o['x'], True), dv(o['gp'], True), torch.from_numpy(o['idx']).to(dev)
        dw, db = torch.full((5, 5, cin, cout), 7.0, device=dev), torch.full((cout,), 7.0, device=dev)
        with per_call_env(case.get('env')):
            ops.conv2d_wgrad_unpool(xd, gd, idd, 5, dw, db=db)
        out += [('dw', dw), ('db', db)]
        what = 'ops.conv2d_wgrad_unpool(per-call env {})'.format(case.get('env') or {})
    elif kind == 'epi':
        xd, wd, bd = dv(o['x'], True), dv(o['w']), dv(o['b'])
        y, cp = ops.conv2d(xd, wd, bd, act='leaky_relu', bf16_copy=True)
        out += [('y_copy', y), ('cp_copy', cp)]
        if case['shape'][5] == 3:
            y, cp = ops.conv2d(xd, wd, bd, residual=dv(o['r']), bf16_copy=True)
            out += [('y_res', y), ('cp_res', cp)]
            y, cp = ops.conv2d(xd, wd, bd, bf16_copy=True, copy_lrelu=True)
            out += [('y_plain', y), ('cp_lrelu', cp)]
            out.append(('y_d2s', ops.conv2d(xd, wd, bd, d2s_out=True)))
            out.append(('dx_s2d', ops.conv2d_dgrad(xd, dv(o['w2']), case['shape'][1:3], s2d_out=True)))
        for key, t in out:
            assert t is not None, key + ': the epilogue was not fused'
        what = 'ops.conv2d(x bf16, k {}: leaky_relu + bf16_copy{})'.format(
            case['shape'][5], '; residual + bf16_copy; bf16_copy + copy_lrelu; d2s_out; conv2d_dgrad s2d_out' if case['shape'][5] == 3 else '')
    elif kind == 'convt':
        out.append(('y', ops.convt2x2(dv(o['x'], True), dv(o['w']), dv(o['b']), out_bf16=ob)))
        what = 'ops.convt2x2(x bf16, out_bf16={})'.format(ob)
    elif kind == 'cconv3':
        y, c4 = ops.cconv3(dv(o['x']), dv(o['w']), pad_mode=1, want_c4=True)
        out += [('y', y), ('c4', c4)]
        what = 'ops.cconv3(pad_mode=1, want_c4=True)'
    elif kind == 'conv1':
        n, h, w = case['shape']
        c4 = torch.ones((n, h, w, 4), dtype=BF, device=dev)
        c4[..., :3] = dv(o['x'], True)
        c4 = c4.contiguous()
        for act, tag in (('leaky_relu', '_lrelu'), (None, '')):
            pooled, idx = ops.conv1_pool_c4(c4, dv(o['w']), dv(o['b']), act=act, out_bf16=ob)
            out += [('pooled' + tag, pooled), ('idx' + tag, idx)]
        what = 'ops.conv1_pool_c4(out_bf16={})'.format(ob)
    else:
        raise KeyError(kind)
    torch.cuda.synchronize()
    return out, what


def _run_wgrad(case, ops, dev, dv, o):
    n, h, w, c1, c2, cout, k, s = case['shape']
    pad_mode, xb, zb = case.get('pad_mode', 0), case.get('xb', False), case.get('zb', False)
    x1, x2, dzd = dv(o['x'][..., :c1], xb), (dv(o['x'][..., c1:], xb) if c2 else None), dv(o['dz'], zb)
    kw = dict(x2=x2, stride=s, pad_mode=pad_mode, side=bool(case.get('side')))
    if pad_mode:
        kw['pads'] = ((k - 1) // 2, (k - 1) // 2)
    shape = (k, k, c1 + c2, cout)
    keep = []

    def fresh(fill):
        """A dw buffer holding `fill`; misaligned: 4 bytes past a 16-byte boundary (the ticket finish must step aside)."""
        if case.get('misaligned'):
            flat = torch.zeros(int(np.prod(shape)) + 4, device=dev)
            keep.append(flat)
            t = flat[1:1 + int(np.prod(shape))].view(shape)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = torch.empty(shape, device=dev)
        t.copy_(fill if torch.is_tensor(fill) else torch.full(shape, float(fill), device=dev))
        return t

    def launch(dw, db, accumulate=False):
        with per_call_env(case.get('env')):
            ops.conv2d_wgrad(x1, dzd, k, dw=dw, db=db, accumulate=accumulate, **kw)
        if case.get('side'):
            ops.join_side_stream()

    def body():
        res = []
        for tag in ('', '_again'):                      # the same launch twice into fresh outputs: the same bytes
            dw = fresh(7.0)
            db = None if case.get('no_db') else torch.full((cout,), 7.0, device=dev)
            launch(dw, db)
            res.append(('dw' + tag, dw))
            if db is not None:
                res.append(('db' + tag, db))
        if not case.get('full'):
            acc = fresh(dv(o['dw0']))
            dba = None if case.get('no_db') else dv(o['db0'])
            launch(acc, dba, accumulate=True)
            res.append(('dw_acc', acc))
            if dba is not None:
                res.append(('db_acc', dba))
        return res

    if case.get('small_binding'):
        # a stream whose binding is too small for the launch: the library must fall back to slabs + the reduction launch
        from neural_imaging_amd import _lib
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            small = torch.zeros(16, dtype=torch.uint8, device=dev)
            ops._TICKETS[(dev.index, ops._stream())] = small
            _lib.call('nimg_bind_tickets', ops._stream(), small.data_ptr(), small.numel())
            res = body()
        torch.cuda.current_stream(dev).wait_stream(st)
        keep.append(st)
    else:
        res = body()
    torch.cuda.synchronize()
    res = [(key, t.clone()) for key, t in res]
    what = 'ops.conv2d_wgrad(x {}, dz {}, k {}, stride {}, twice + accumulate{}{}{}, per-call env {})'.format(
        'bf16' if xb else 'f32', 'bf16' if zb else 'f32', k, s, ', side=True + join' if case.get('side') else '',
        ', dw 4 bytes off' if case.get('misaligned') else '', ', 16-byte ticket binding' if case.get('small_binding') else '', case.get('env') or {})
    return res, what


def host(t):
    """A result tensor as the numpy array the .npz holds (bf16 widened to float32: the same value)."""
    t = t.detach()
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def expected_keys(group):
    keys = set()
    for c in GROUPS[group]['cases']:
        keys |= {c['name'] + '/' + k for k in reference_keys(c)}
        if group in TICKET_GROUPS:
            keys |= {c['name'] + '/tickets', c['name'] + '/bound_streams'}
    return keys


def reference_keys(case):
    """The keys of reference(case) without computing it."""
    kind, full, no_db = case['kind'], bool(case.get('full')), bool(case.get('no_db'))
    if kind == 'fwd':
        return ['y'] if full else ['y_lrelu'] if case.get('lrelu_only') else ['y', 'y_lrelu']
    if kind == 'dgrad':
        return ['dx'] if (full or case.get('split')) else ['dx', 'dx_mask']
    if kind in ('pool', 'conv1'):
        return ['pooled_lrelu', 'idx_lrelu'] + ([] if case.get('lrelu_only') else ['pooled', 'idx'])
    if kind == 'and_pool':
        return ['y', 'pooled', 'y_lrelu', 'pooled_lrelu']
    if kind == 'dgrad_unpool':
        return ['dx', 'fold_ok'] if full else ['dx', 'dx_mask', 'fold_ok']
    if kind == 'wgrad':
        keys = ['dw', 'dw_again'] + ([] if no_db else ['db', 'db_again'])
        return keys if full else keys + ['dw_acc'] + ([] if no_db else ['db_acc'])
    if kind == 'wgrad_unpool':
        return ['dw', 'db']
    if kind == 'convt':
        return ['y']
    if kind == 'epi':
        return ['y_copy', 'cp_copy'] + (['y_res', 'cp_res', 'y_plain', 'cp_lrelu', 'y_d2s', 'dx_s2d'] if case['shape'][5] == 3 else [])
    if kind == 'cconv3':
        return ['y', 'c4']
    raise KeyError(kind)


def compare(case, got, what=''):
    """got: {key: array} of ONE case.  Integer cases: == against the float64 reference (arg-max bytes too); full-mantissa cases: the
    project's tolerances, and a launch repeated must give the same bytes."""
    from util import assert_exact
    ref = reference(case)
    assert set(ref) <= set(got), '{}: missing {}'.format(case['name'], sorted(set(ref) - set(got)))
    worst = {}
    for key, want in ref.items():
        name = '{}{}/{}'.format(what, case['name'], key)
        if want.dtype == np.uint8:
            assert got[key].dtype == np.uint8 and got[key].shape == want.shape and np.array_equal(got[key], want), \
                '{}: {} of {} bytes differ'.format(name, int((got[key] != want).sum()) if got[key].shape == want.shape else -1, want.size)
        elif case.get('full'):
            worst[key] = check_full(name, got[key], want, stores_bf16(case, key))
        else:
            assert_exact(got[key], want, name)
    if case['kind'] == 'wgrad':
        for a, b in (('dw', 'dw_again'), ('db', 'db_again')):
            if a in got:
                assert got[a].tobytes() == got[b].tobytes(), '{}{}: the launch repeated gives other bytes ({})'.format(what, case['name'], a)
    return worst


def assert_counters_zero(name, tickets):
    """The counter buffers of every bound stream, read back whole after a case: the last arriver of every tile stored 0 again."""
    tickets = np.asarray(tickets)
    assert tickets.dtype == np.uint8 and tickets.size >= 64 * 1024, '{}: {} counter bytes read back'.format(name, tickets.size)
    assert not tickets.any(), '{}: {} counter bytes are not zero after the launches'.format(name, int(np.count_nonzero(tickets)))


BY_NAME = {}
for _case in all_cases():
    assert _case['name'] not in BY_NAME, 'duplicate case name ' + _case['name']
    BY_NAME[_case['name']] = _case
