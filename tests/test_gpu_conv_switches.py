"""
Exact tests of the convolution routes behind process-wide switches and of the in-kernel split-K finish ("tickets").

csrc/ reads most NIMG_* switches of the convolution files once per process (static const ... = getenv(...)), so the kernels
behind them cannot be toggled inside the pytest process that runs tests/test_gpu_exact.py.  Three kinds of code sit there: the
FALLBACK kernels that are the product path for tensors above 2 GB (every buffer-load / LDS-DMA / ring route carries a
`bytes < 2^31 - 65536` condition; the NIMG_NO_* switches are the only way to reach what lies behind it at a small shape), the OPT-IN
forms that ship in the library and that tools/ times against the default, and the ticket finish of common.h.  Each GROUP of
conv_cases.GROUPS runs in ONE fresh child process (tests/conv_child.py) started with exactly that group's variables; the child
writes every result tensor to an .npz and compares nothing; this module compares each with the float64 reference of
conv_cases.reference(): `==` on integer operands (assert_exact, arg-max bytes with np.array_equal), the tolerances of
test_gpu_exact.test_full_mantissa_* on full-mantissa operands (2e-5 max|ref| for float32 outputs, 2^-8 |ref| + 2e-5 max|ref| for
bf16 outputs), and it asserts that every expected key is present.  Children run one after the other, each under a 240 s limit,
never retried; after a child that ended by a signal, a timeout, status 134 / 139 or with a HIP illegal memory access in its
stderr no further child is started (every later group test fails at once).

Tickets run in children too: once nimg_bind_tickets has bound a stream the library finishes every weight gradient launched on it
in the kernel, whatever ops.TICKETS says later - an in-process test would move every later test of the pytest process onto that path.
In both ticket groups dw, db and the accumulated dw / db must equal wgrad_ref, the same launch repeated must give the same bytes,
and the whole counter buffer of every bound stream must be zero after every case.  The generic kernel's item map counts whole
float4 only (c4n = min(TCO, Cout - co0) >> 2): the entry point refuses Cout % 4 != 0 (NIMG_ERR_ARG in wgrad_bf16_impl) and ops
routes such layers to the float32 path, so no tail channel exists; tk-generic-k3-8to4-smallest-cout pins the smallest accepted one.

Kernel newly reached by each group (read off the dispatch and confirmed by one rocprofv3 --kernel-trace --stats run of each child:
every kernel named here appears in its group's trace, the ticket cases with grids of blocks_io x slabs workgroups and without a
reduce_slabs2_kernel launch except for the fall-backs; the ids are the case names of conv_cases.py, grouped by prefix).  The trace
corrected two readings: nimg_conv2d_fwd_pool_bf16 chooses the 32-channel tile below 384 workgroups of 64 channels whatever
NIMG_TN32_BELOW says, so the pooling epilogue of the 64-channel tiles and of the rings runs at 48 images (*-384wg), and a 3x3 layer
of at most 1024 pixels goes to the LDS-DMA tile before the 3x3 ring is asked (ring3-32to128-ragged-1600px).

  plain           conv_fwd_bf16_kernel<3|5, 1, 16, 16, 1, 32|64, INB, BUF = false> with one and two bf16 inputs (plain-tn*), its 8x8x4 form
                  (plain-8x8x4-*), the 32x16 tile <5, 1, 32, 16, 1, 32, INB> at 2048 tiles and 8 output channels (plain-32x16-*), its pooling (TN32 below 384 workgroups, TN64 at 384) / pool_also epilogues and masks; ops.unpool_fold_ok is False and the materialising
                  form (maxpool2_unpool + conv2d_dgrad) is exact (plain-unpool-materialised-*)
  fallbacks       buffer-load tiles <..., INB, BUF = true> at the LDS-DMA shapes (buf-*-dma-shape, buf-8x8x4-*) and at the ring shapes
                  with and without un-pooling (buf-tn64-k5-*, buf-pool-*, buf-dgrad-*, buf-unpool-*: <5, 1, 16, 16, 1, 32|64, true, true, true>),
                  1x1 with 16-channel chunks at Cin % 64 == 0 (k1-ck16-*), conv_wgrad_bf16_kernel<3, 1, 4, true, true> at 8 x 8 images
                  (generic-8x8-*), its 64-wide dz tile at Cout <= 32 (wide-dz-tile-*), <5, 1, 8, true, true, 16, true> from the pooled
                  gradient (generic-unpool-*), conv_wgrad_c3k5_kernel at w % 64 == 0 (c3k5-valu-*), the four-phase convt2x2 (convt-phases-*)
  optin_a         conv5_ring_kernel<128, *, 8> (ring128nw8-*, pooling included), conv5_ring_kernel<128, false, 4, 3> (ring3-*), the tile behind
                  NIMG_NO_CONV5_RING64 (tile-*-ring64-off), conv3_dma_kernel<8, 8, 4, ..., LAY = 0> (dma4-pixel-major-*),
                  conv5_dgrad_sparse16_kernel (sparse16-*), conv5_wgrad_alltaps_kernel<8, true, 1> (wgrad5-8-kx3l-s1-*)
  optin_b         conv5_ring_kernel<64> at Cout % 128 == 0, Hout >= 32 (ring64-*; ring128 below 32 rows: ring128-h24-under-tn64), the
                  buffer-load tile behind NIMG_NO_CONV5_RING32 (buf-tn32-*-ring32-off), conv5_dgrad_sparse_kernel<4> (sparse-block42-*),
                  conv5_wgrad_alltaps_kernel<16, true, 1> (wgrad5-16-kx3l-s1-*), conv_wgrad_c3k5_mfma_kernel<16> (c3k5-mfma16-*),
                  cconv_kernel<64, 1> (cconv-64x1-*), conv3_rows_kernel<1, 128, 4, 1, 4> (rows-ncw4-pfd1-*)
  splits          conv3_wgrad_alltaps_kernel, conv_wgrad_bf16_kernel<5, ...> and the three wgrad5 forms at the largest slab counts their
                  targets accept (work_per_split 1, ragged last split; the dense wgrad5 form as conv5_wgrad_alltaps_kernel<16 | 8, false, 1>),
                  conv3_rows_kernel with 3 workgroups for 9 .. 10 units of 4 rows and its 4-wave form <1, 128, 4, 2, 4> (rows-*), cconv_kernel / conv1_pool_fwd_kernel with more tiles than
                  workgroups (cconv-cap256-*, conv1-cap256-*), the buffer-load tile where NIMG_CONV3_DMA_MAXHW = 0 refuses the DMA tile
  tickets         ticket_finish in conv_wgrad_bf16_kernel (tk-generic-*: k = 1, 3, 5, 2x2 / stride 2, stride-2 5x5, float32 and bf16
                  operands, 1 / 2 / 24 / 25 / 27 slabs), its pair8 form (tk-pair8-*, n odd and even) and conv3_wgrad_alltaps_kernel at
                  NB = 1, 2, 4 (tk-alltaps3-*); db null; the fall-backs to slabs (dw 4 bytes off a 16-byte boundary, a 16-byte
                  binding); side streams with a buffer each
  tickets_splits  the two-level finish at 68 .. 144 slabs (groups of 9 / 12, a ragged last group) under NIMG_WGRAD3_BLOCKS
  no_tickets      NIMG_NO_TICKETS beside NIMG_TICKETS: streams bound as in `tickets`, every launch takes the slabs and the reduction
                  launch all the same (ntk-*); conv5_wgrad_alltaps_kernel<16 | 8, true, 2> (wgrad5-*-kx3l-s2-*) - with the groups above
                  and tests/test_gpu_exact.py all eight launch<TH, KX3L, SCHED> combinations of wgrad5.hip

Epilogues beyond bias / activation / mask / pooling (conv_cases.epi: *-epilogues*): the 5x5 rings know none of them and the dispatch
steps aside to the tile kernel (plain_epi) - a LeakyReLU + bf16-copy layer at a ring shape runs in every group that switches a 5x5
ring on or off (tile-behind-ring128nw8-*, tile-behind-ring64-*, buf-tn64-k5-epilogues-*, plain-*-epilogues); the 3x3 ring ends in the
tile kernel's own conv_epilogue_vec (called with wm = wave, wn = 0, as no other kernel calls it) and takes residual + bf16 copy,
copy_lrelu, the depth-to-space store and the space-to-depth store of an input gradient itself (ring3-epilogues-128to128).

In-process (no child): the switches csrc/ reads per call - NIMG_NO_WGRAD3_ALLTAPS (conv_wgrad_bf16_kernel at the alltaps3 shapes)
and NIMG_WGRAD3_NB = 1 | 2 at Cout % 128 == 0 (conv3_wgrad_alltaps_kernel<1, 16>, <1, 8>, <2, 8>) - and ops.REDUCE_STREAM.

Not reached, with the reason:
  NIMG_CONV3_STAGES / PIPE / ILV / LOADER, PLANES = 2      compiled out of the default build (NIMG_CONV3_VARIANTS)
  NIMG_ROWS_ABLATE, NIMG_C5C3_ABL                          leave parts of the layer out by design; NIMG_ROWS_RB is a dead read
"""
import os
import signal
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import conv_cases as C
from util import assert_exact

pytestmark = pytest.mark.gpu

_T0 = [None]
_FAULTED = []                      # the first child that faulted: no further child is started
_CHILD_SECONDS = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    _T0[0] = time.monotonic()
    yield torch.device('cuda', 0)
    print('conv switches: module wall time {:.1f} s, children {}'.format(
        time.monotonic() - _T0[0], ', '.join('{} {:.1f} s'.format(g, s) for g, s in _CHILD_SECONDS.items())))       # (pytest -s)


def child_env(group, base=None):
    """The child's environment: the parent's without any NIMG_* name, plus the group's variables."""
    env = {k: v for k, v in (os.environ if base is None else base).items() if not k.startswith('NIMG_')}
    env.update(C.GROUPS[group]['env'])
    return env


def faulted(returncode, stderr):
    """Did a child end the way a GPU fault ends one?  (a signal, abort / segmentation fault statuses, HIP's illegal access)"""
    return returncode < 0 or returncode in (134, 139, 128 + signal.SIGABRT, 128 + signal.SIGSEGV, 124, 137) or \
        'illegal memory access' in stderr or 'Memory access fault' in stderr


def run_child(group, out_dir):
    assert not _FAULTED, 'not started: child {} faulted earlier in this module'.format(_FAULTED[0])
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_child.py')
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, child, group, str(out_dir)], env=child_env(group), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=240)
    except subprocess.TimeoutExpired:
        _FAULTED.append(group)
        raise AssertionError('child {} ran into its time limit'.format(group))
    _CHILD_SECONDS[group] = time.monotonic() - t0
    err = p.stderr.decode(errors='replace')
    if faulted(p.returncode, err):
        _FAULTED.append(group)
    assert p.returncode == 0, 'child {} failed ({}): {}'.format(group, p.returncode, err[-3000:])
    lines = p.stdout.decode().splitlines()
    done = [l.split(':', 1)[0] for l in lines if ':' in l]
    assert done == [c['name'] for c in C.GROUPS[group]['cases']], 'child {} ran {}'.format(group, done)
    with np.load(os.path.join(str(out_dir), group + '.npz')) as z:
        return {k: z[k] for k in z.files}


def check_group(group, got):
    """Every expected key present, every tensor equal to the reference; ticket groups: every counter word zero again."""
    missing = C.expected_keys(group) - set(got)
    assert not missing, 'child {} left out {}'.format(group, sorted(missing))
    failures, measured, bound = [], [], 0
    for case in C.GROUPS[group]['cases']:
        mine = {k.split('/', 1)[1]: v for k, v in got.items() if k.split('/', 1)[0] == case['name']}
        try:
            worst = C.compare(case, mine, what=group + ': ')
            measured += ['conv switches: full mantissa {}/{}: error / tolerance {:.3f}'.format(case['name'], k, v) for k, v in worst.items()]
            if group in C.TICKET_GROUPS:
                C.assert_counters_zero(case['name'], mine['tickets'])
                now, before = int(mine['bound_streams'][0]), bound
                bound = now
                if case.get('side') and case['name'].endswith('-side-streams') and 'alltaps3' not in case['name']:
                    # the group's first side=True case: both side streams are new and bind a counter buffer each
                    assert before >= 1 and now >= before + 2, '{}: {} streams bound, {} before'.format(case['name'], now, before)
            if case['name'] in TWINS or case['name'] in TWINS.values():
                _FULL_DW[case['name']] = mine['dw']
        except AssertionError as e:
            failures.append('{}: {}'.format(case['name'], str(e)[:1500]))
    print('\n'.join(measured))
    assert not failures, '{} of {} cases of group {} differ:\n'.format(len(failures), len(C.GROUPS[group]['cases']), group) + '\n'.join(failures)


@pytest.mark.parametrize('group', list(C.GROUPS))
def test_switch_group_in_a_fresh_process(dev, group, tmp_path):
    check_group(group, run_child(group, tmp_path))


# The same full-mantissa weight gradient under NIMG_TICKETS and under NIMG_TICKETS + NIMG_NO_TICKETS.  Integer results cannot tell the
# in-kernel finish from the slab reduction; these can: ticket_sum adds the 25 / 27 slabs in groups of 5 / 6 in split order and then
# the group sums, reduce_slabs adds slabs k and k + 16 in 16 segments and then the segments - two roundings of the same sum, both
# inside the tolerance, that agree in every one of the ~10^4 elements only if a group took the other group's path.
TWINS = {'tk-full-generic': 'ntk-full-generic', 'tk-full-alltaps3': 'ntk-full-alltaps3'}
_FULL_DW = {}


@pytest.mark.parametrize('name', list(TWINS))
def test_ticket_finish_and_slab_reduction_are_two_summation_orders(dev, name):
    assert name in _FULL_DW and TWINS[name] in _FULL_DW, 'the ticket groups did not run before this test'
    a, b = _FULL_DW[name], _FULL_DW[TWINS[name]]
    assert a.shape == b.shape and a.tobytes() != b.tobytes(), \
        '{}: byte-identical with and without NIMG_NO_TICKETS - one of the two groups did not take its path'.format(name)


# ----------------------------------------------------------------------------------------------------------------------
# the switches csrc/ reads on every call, and ops.REDUCE_STREAM: inside this process
@pytest.mark.parametrize('case', [pytest.param(c, id=c['name']) for c in C.PER_CALL_CASES])
def test_per_call_switch_exact(dev, case, monkeypatch):
    """NIMG_NO_WGRAD3_ALLTAPS: the generic kernel at the alltaps3 shapes, two-input ones included; NIMG_WGRAD3_NB = 1 | 2 at
    Cout % 128 == 0 with h % 16 == 0 and h % 16 == 8: conv3_wgrad_alltaps_kernel<1, 16>, <1, 8>, <2, 8> at shapes the default
    (NB = 4) never gives them."""
    from neural_imaging_amd import ops
    assert not _FAULTED, 'not started: child {} faulted earlier in this module'.format(_FAULTED[0])
    assert not ops.TICKETS and not ops._TICKETS, 'the ticket finish must stay out of the pytest process'
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    tensors, _ = C.run(case, ops, dev)
    C.compare(case, {k: C.host(t) for k, t in tensors})


def test_reduce_stream_exact(dev, monkeypatch):
    """ops.REDUCE_STREAM: three side=True weight gradients whose slab reductions run on the side streams' reduction streams, then
    ONE join: dw and db equal the reference."""
    from neural_imaging_amd import ops
    assert not _FAULTED, 'not started: child {} faulted earlier in this module'.format(_FAULTED[0])
    assert ops._SIDE['enabled'] and not ops.DEFER_REDUCE and not ops.CHAIN_REDUCE
    monkeypatch.setattr(ops, 'REDUCE_STREAM', True)
    ops.set_compute('bf16')
    dv = lambda a, bf: (lambda t: t.to(torch.bfloat16) if bf else t)(torch.from_numpy(np.array(a, dtype=np.float32, order='C')).to(dev).contiguous())
    pending = []
    for case in C.REDUCE_STREAM_CASES:
        n, h, w, c1, c2, cout, k, s = case['shape']
        o = C.operands(case)
        dw, db = torch.full((k, k, c1, cout), 7.0, device=dev), torch.full((cout,), 7.0, device=dev)
        ops.conv2d_wgrad(dv(o['x'], case.get('xb', False)), dv(o['dz'], case.get('zb', False)), k, stride=s, dw=dw, db=db, side=True)
        pending.append((case, dw, db))
    assert ops._RSTREAM['dirty'], 'no reduction went to a reduction stream'
    ops.join_side_stream()
    torch.cuda.synchronize()
    for case, dw, db in pending:
        ref = C.reference(case)
        assert_exact(C.host(dw), ref['dw'], case['name'] + ' dw')
        assert_exact(C.host(db), ref['db'], case['name'] + ' db')
