"""
The parts of tests/test_gpu_conv_switches.py that need no GPU: the inventory of getenv("NIMG_...") reads under csrc/ against
conv_cases.SWITCHES (a switch added later cannot go untested silently), the grouping rules, the restatement of the split-K plans
that chooses the ticket shapes, every reference half with its exact-arithmetic conditions, and the proof that the comparisons can
fail: float32 numpy stand-ins for the ticket finish and for two fallback kernels, each with one defect, must be rejected.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import tfops as T

import conv_cases as C
import test_gpu_conv_switches as M
from util import to64, unpool

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neural-imaging_amd', 'csrc')
GETENV = re.compile(r'getenv\("(NIMG_[A-Z0-9_]+)"\)')


def scan(csrc=CSRC):
    """{name: [(file, line text)]} of every getenv("NIMG_...") in csrc/*.hip and csrc/*.h."""
    found = {}
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith(('.hip', '.h')):
            with open(os.path.join(csrc, fn)) as f:
                for line in f:
                    for name in GETENV.findall(line):
                        found.setdefault(name, []).append((fn, line))
    return found


def inventory_errors(found, switches):
    errs = ['{} is read in csrc/{} and has no SWITCHES entry'.format(n, found[n][0][0]) for n in sorted(set(found) - set(switches))]
    errs += ['SWITCHES names {}, which csrc/ no longer reads'.format(n) for n in sorted(set(switches) - set(found))]
    for n, st in sorted(switches.items()):
        head, _, rest = st.partition(':')
        if head not in ('group', 'per_call', 'covered_elsewhere', 'excluded') or (head != 'per_call' and not rest.strip()):
            errs.append('{}: status {!r} is malformed or has an empty reason'.format(n, st))
    return errs


def test_every_switch_of_csrc_is_in_the_inventory():
    found = scan()
    assert len(found) >= 45
    assert inventory_errors(found, C.SWITCHES) == []
    # the check itself can fail: a new read, a stale entry, an excluded entry without a reason
    more = dict(found, NIMG_X=[('conv_bf16.hip', 'static const bool x = getenv("NIMG_X") != nullptr;')])
    assert any('NIMG_X' in e for e in inventory_errors(more, C.SWITCHES))
    assert any('NIMG_GONE' in e for e in inventory_errors(found, dict(C.SWITCHES, NIMG_GONE='group:plain')))
    assert any('NIMG_ROWS_RB' in e for e in inventory_errors(found, dict(C.SWITCHES, NIMG_ROWS_RB='excluded:')))
    assert any('NIMG_ROWS_RB' in e for e in inventory_errors(found, dict(C.SWITCHES, NIMG_ROWS_RB='skipped:because')))


def test_statuses_agree_with_the_sources_and_the_groups():
    found = scan()
    assert len(C.GROUPS) <= 8
    set_somewhere = {}
    for g, spec in C.GROUPS.items():
        for name in spec['env']:
            assert name in C.SWITCHES or name == 'NIMG_TICKETS', name           # (NIMG_TICKETS is read by ops.py, not by csrc/)
            set_somewhere.setdefault(name, set()).add(g)
    per_call_used = {k for c in C.all_cases() for k in (c.get('env') or {})}
    for name, st in C.SWITCHES.items():
        head, _, rest = st.partition(':')
        # read once: every read initialises a function-local `static const` (or continues the initialiser of one on the next line)
        once = all('static const' in line or line.lstrip().startswith('getenv(') for _, line in found[name])
        if head == 'group':
            assert once, '{} is read per call: it needs no child'.format(name)
            assert set(rest.split(',')) == set_somewhere.get(name), (name, rest, set_somewhere.get(name))
        elif head == 'per_call':
            assert not once and name in C.PER_CALL and name in per_call_used, name
        elif head == 'covered_elsewhere':
            assert os.path.exists(os.path.join(os.path.dirname(__file__), rest + '.py'))
            with open(os.path.join(os.path.dirname(__file__), rest + '.py')) as f:
                assert name in f.read()
        else:
            assert name not in set_somewhere and name not in per_call_used
    assert set(C.PER_CALL) == {n for n, st in C.SWITCHES.items() if st == 'per_call'}
    # one switch must not mask the route another of its group opens
    for a, b in (('NIMG_RING_TN64', 'NIMG_NO_CONV5_RING64'), ('NIMG_NO_CONV5_RING', 'NIMG_RING_NW8'), ('NIMG_NO_BUFFER_LOADS', 'NIMG_NO_CONV3_DMA'),
                 ('NIMG_NO_WGRAD5_ALLTAPS', 'NIMG_WGRAD5_KX3L'), ('NIMG_DGRAD5S_ACC16', 'NIMG_DGRAD5S_BLOCK42'), ('NIMG_NO_C3K5_MFMA', 'NIMG_C3K5_TR8'),
                 ('NIMG_NO_CONV5_RING', 'NIMG_NO_CONV5_RING32'), ('NIMG_NO_BUFFER_LOADS', 'NIMG_CONV3_RING_MIN')):
        assert not (set_somewhere[a] & set_somewhere[b]), (a, b)
    # every case of a group has a name of its own, and every group sets what the child will find
    assert M.child_env('plain', {'NIMG_TICKETS': '1', 'NIMG_FOO': '2', 'HOME': '/h', 'PATH': '/p'}) == \
        dict(C.GROUPS['plain']['env'], HOME='/h', PATH='/p')
    assert sum(len(s['cases']) for s in C.GROUPS.values()) == len({c['name'] for s in C.GROUPS.values() for c in s['cases']})


def test_a_faulted_child_stops_the_module(tmp_path, monkeypatch):
    assert M.faulted(-11, '') and M.faulted(-6, '') and M.faulted(134, '') and M.faulted(139, '') and M.faulted(1, 'HIP error: an illegal memory access was encountered')
    assert not M.faulted(1, 'AssertionError') and not M.faulted(0, '')
    monkeypatch.setattr(M, '_FAULTED', ['optin_a'])
    with pytest.raises(AssertionError, match='not started'):
        M.run_child('optin_b', tmp_path)


def test_split_plans_give_the_intended_slab_counts():
    assert [C.ticket_group(s) for s in (1, 2, 24, 25, 27, 68, 144)] == [1, 2, 24, 5, 6, 9, 12]
    counts = set()
    for g, blocks in (('tickets', 256), ('tickets_splits', int(C.BIG)), ('no_tickets', 256)):
        for c in [c for c in C.GROUPS[g]['cases'] if c['kind'] == 'wgrad']:
            assert C.ticket_slabs(c, blocks) == c['slabs'], c['name']
            counts.add(c['slabs'])
            tiles = C.cdiv(c['shape'][3] + c['shape'][4], 32) * C.cdiv(c['shape'][5], 32)
            groups = C.cdiv(c['slabs'], C.ticket_group(c['slabs']))
            assert tiles * (1 + groups) * 4 <= 64 * 1024, c['name']                 # the bound buffer holds the counters
    assert {1, 2, 24, 25, 27, 68, 144} <= counts
    assert 27 % C.ticket_group(27) and 68 % C.ticket_group(68)                   # ragged last groups
    by = C.BY_NAME
    assert C.alltaps3_plan(by['tk-alltaps3-nb1-th16-32to32'])[:2] == (1, 16) and C.alltaps3_plan(by['tk-alltaps3-nb1-th8-25slabs'])[:2] == (1, 8)
    assert C.alltaps3_plan(by['tk-alltaps3-nb2-32+32to64'])[:2] == (2, 8) and C.alltaps3_plan(by['tk-alltaps3-nb4-64to128'])[:2] == (4, 8)
    assert C.alltaps3_plan(by['tk-generic-k3-bf16-both-w24']) is None           # w % 16 != 0: the generic kernel with bf16 operands
    # NIMG_WGRAD3_BLOCKS / NIMG_WGRAD5_BLOCKS change the count where the group 'splits' says so
    for c in C.SPLITS:
        if 'plan' in c:
            assert C.alltaps3_plan(c, int(C.BIG)) == c['plan'] and C.alltaps3_plan(c, 256) == c['plan_default'], c['name']
        if 'slabs' in c:
            assert C.generic_splits(c, 512) == c['slabs'] and C.generic_splits(c, 256) == c['slabs_default'], c['name']
    assert any(c.get('plan') != c.get('plan_default') for c in C.SPLITS) and any(c.get('slabs') != c.get('slabs_default') for c in C.SPLITS)
    # the per-call cases reach the instantiations their names say
    want = {'alltaps3-nb1-th16-at-128-channels': (1, 16), 'alltaps3-nb1-th8-at-128-channels': (1, 8),
            'alltaps3-nb2-th8-at-128-channels-h32': (2, 8), 'alltaps3-nb2-th8-at-128-channels-h24': (2, 8)}
    for name, plan in want.items():
        assert C.alltaps3_plan(by[name])[:2] == plan and by[name]['shape'][5] % 128 == 0


@pytest.mark.parametrize('group', list(C.GROUPS) + ['in-process'])
def test_reference_halves_and_their_conditions(group):
    """Every reference runs without a GPU; reference() asserts the two exact-arithmetic conditions (util.assert_exact_conditions)
    on every integer case.  The keys are the ones the parent demands of the child; results stay near 2 MB."""
    cases = C.GROUPS[group]['cases'] if group in C.GROUPS else C.PER_CALL_CASES + C.REDUCE_STREAM_CASES
    for c in cases:
        ref = C.reference(c)
        assert set(ref) == set(C.reference_keys(c)), c['name']
        for k, v in ref.items():
            # (about 2 MB as float32; the pooled tensor of 384 workgroups of 64 channels - what the 64-channel pooling routes need -
            #  is 6.3 MB, the 2048 tiles of 32 x 16 pixels x 8 channels of the 32x16 tile 34 MB: 8 MB of bf16 on the device)
            limit = 34e6 if '2048tiles' in c['name'] else 6.3e6 if c.get('lrelu_only') else 2.4e6
            assert v.size * (1 if v.dtype == np.uint8 else 4) <= limit, (c['name'], k, v.shape)
            if not c.get('full') and v.dtype != np.uint8:
                assert np.array_equal(v, np.asarray(v, np.float32).astype(np.float64))
    if group in C.GROUPS:
        keys = C.expected_keys(group)
        assert len(keys) >= 2 * len(cases) and (group not in C.TICKET_GROUPS or sum(k.endswith('/tickets') for k in keys) == len(cases))
    assert len(C.GROUPS) == 8


# ----------------------------------------------------------------------------------------------------------------------
# the comparisons can fail
def _slabs(ref, splits, seed):
    """float32 slabs of small integers that sum to ref (what `splits` workgroups would have written)."""
    s = np.random.default_rng(seed).integers(-3, 4, size=(splits,) + ref.shape).astype(np.float32)
    s[-1] = (ref - s[:-1].astype(np.float64).sum(axis=0)).astype(np.float32)
    return s


def ticket_stand_in(slabs, dst, accumulate, defect=None):
    """common.h ticket_finish in float32 numpy: groups of ticket_group(splits) slabs summed in split order, then the group sums in
    group order, onto dst when accumulating.  Returns (result, counter words)."""
    splits = slabs.shape[0]
    G = C.ticket_group(splits)
    NG = C.cdiv(splits, G)
    sums = []
    for g in range(NG):
        members = list(range(g * G, min(splits, (g + 1) * G)))
        if defect == 'slab twice' and g == 0:
            members.append(members[0])
        acc = slabs[members[0]].copy()
        for k in members[1:]:
            acc += slabs[k]
        sums.append(acc)
    if defect == 'last group dropped' and NG > 1:
        sums = sums[:-1]
    out = sums[0].copy()
    for s in sums[1:]:
        out += s
    if accumulate and defect != 'accumulate ignored':
        out += dst
    if defect == 'tail channels dropped':
        out[..., -(out.shape[-1] % 4 or 2):] = dst[..., -(out.shape[-1] % 4 or 2):]
    counters = np.zeros(64 * 1024, np.uint8)
    if defect == 'counter left':
        counters[4 * (1 + NG - 1)] = 1
    return out, counters


@pytest.mark.parametrize('name', ['tk-generic-k3-24to40-27slabs', 'tk-generic-k3-24to40-24slabs', 'tk-alltaps3-nb1-th8-25slabs'])
def test_ticket_comparisons_reject_a_wrong_finish(name):
    case = C.BY_NAME[name]
    o, ref = C.operands(case), C.reference(case)

    def got(defect):
        out, counters = {}, None
        for key, fill in (('dw', None), ('db', None), ('dw_acc', o['dw0']), ('db_acc', o['db0'])):
            base = ref['dw'] if key.startswith('dw') else ref['db']
            dst = np.full(base.shape, 7.0, np.float32) if fill is None else fill.astype(np.float32)
            out[key], counters = ticket_stand_in(_slabs(base, case['slabs'], 5), dst, fill is not None, defect)
        out['dw_again'], out['db_again'] = out['dw'].copy(), out['db'].copy()
        return out, counters

    good, counters = got(None)
    C.compare(case, good)
    C.assert_counters_zero(name, counters)
    for defect in ('last group dropped', 'slab twice', 'tail channels dropped', 'accumulate ignored'):
        if defect == 'last group dropped' and case['slabs'] <= 24:
            continue
        with pytest.raises(AssertionError):
            C.compare(case, got(defect)[0])
    with pytest.raises(AssertionError, match='not zero'):
        C.assert_counters_zero(name, got('counter left')[1])
    with pytest.raises(AssertionError, match='read back'):
        C.assert_counters_zero(name, np.zeros(16, np.uint8))
    other = dict(good, dw_again=good['dw'] + np.float32(0))
    other['dw_again'][0, 0, 0, 0] = np.float32(-0.0) if good['dw'][0, 0, 0, 0] == 0 else -good['dw'][0, 0, 0, 0]
    with pytest.raises(AssertionError):
        C.compare(case, other)
    with pytest.raises(AssertionError, match='missing'):
        C.compare(case, {k: v for k, v in good.items() if k != 'db_acc'})


def _conv32(x, w, b=None):
    return T.conv2d(torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(w, np.float32)),
                    None if b is None else torch.from_numpy(np.asarray(b, np.float32))).numpy()


def test_fallback_comparisons_reject_a_wrong_kernel():
    # the un-pooling input gradient: a stand-in that ignores the arg-max bytes (routes every gradient to window position 0)
    case = C.BY_NAME['buf-unpool-tn64-128from64-f32out']
    o, ref = C.operands(case), C.reference(case)
    from util import mask_f32
    dx = _conv32(unpool(o['gp'], o['idx']), C.flipped(o['w']))
    good = {'dx': dx, 'dx_mask': mask_f32(dx.astype(np.float64), o['m']), 'fold_ok': np.uint8([1])}
    C.compare(case, good)
    bad = _conv32(unpool(o['gp'], np.zeros_like(o['idx'])), C.flipped(o['w']))
    with pytest.raises(AssertionError):
        C.compare(case, dict(good, dx=bad))
    with pytest.raises(AssertionError):
        C.compare(case, dict(good, fold_ok=np.uint8([0])))
    # a ring kernel that reads one input column of one 16-column tile from the column next to it
    case = C.BY_NAME['ring128nw8-32to128-f32out']
    o, ref = C.operands(case), C.reference(case)
    y = _conv32(o['x'], o['w'], o['b'])
    from util import lrelu_f32
    good = {'y': y, 'y_lrelu': lrelu_f32(y.astype(np.float64))}
    C.compare(case, good)
    x1 = o['x'].copy()
    x1[1, :, 32] = o['x'][1, :, 31]
    assert not np.array_equal(x1, o['x'])
    yb = _conv32(x1, o['w'], o['b'])
    with pytest.raises(AssertionError):
        C.compare(case, dict(good, y=yb))
    # arg-max bytes are compared byte for byte, the tie rule included
    case = C.BY_NAME['buf-tn32-pool-k5-32to128-below-384wg']
    ref = C.reference(case)
    good = {k: (v if v.dtype == np.uint8 else v.astype(np.float32)) for k, v in ref.items()}
    C.compare(case, good)
    from util import first_max_pool, lrelu_f32 as L
    o = C.operands(case)
    full = L(C.conv_ref(o['x'], o['w'], o['b'])[0]).astype(np.float64)
    with pytest.raises(AssertionError, match='bytes differ'):
        C.compare(case, dict(good, idx_lrelu=first_max_pool(full, last=True)[1]))
    # full-mantissa cases: a result accumulated in bf16 precision is outside the tolerance, one in float32 is inside
    case = C.BY_NAME['ring128nw8-full']
    o, ref = C.operands(case), C.reference(case)
    y = _conv32(o['x'], o['w'], o['b'])
    C.compare(case, {'y': y})
    with pytest.raises(AssertionError, match='full mantissa'):
        C.compare(case, {'y': y * np.float32(1 + 2.0 ** -9)})
