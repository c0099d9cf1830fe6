"""
Host checks of the real-codec training forward: its numpy restatement (tests/jpeg_ste_ref.py) against the
restated codec it is cut from, the condition its `saturated` cases have to meet so that a mask of all ones cannot pass, the model
surface of the three straight-through codec names, and the refusals of ops.jpeg_ste_fwd that need no device.  No GPU.
"""
import numpy as np
import pytest
import torch

import jpeg_ref
import jpeg_ste_ref as S
import jpegq_ref
from neural_imaging_amd import ops
from neural_imaging_amd.models.jpeg import JPEG


@pytest.mark.parametrize('case', S.CASES, ids=S.CASE_IDS)
def test_restatement_decodes_the_bytes_of_the_restated_codec(case):
    sub, shape, kind, q = case
    ref = S.reference(*case)
    xb = jpeg_ref.to_bytes(S.image(shape, kind))
    assert np.array_equal(xb, S.convert(S.image(shape, kind)))          # on [0, 1] the operator's conversion is the reference's
    for i in range(shape[0]):
        want = jpegq_ref.compress(xb[i], S.tables_of(q), sub)[1] if q == 'three' else jpeg_ref.compress(xb[i], q, sub)[1]
        assert np.array_equal(ref['u8'][i], want)
    assert ref['y'].dtype == np.float32 and np.array_equal(ref['y'], jpeg_ref.to_float(ref['u8']))
    # the mask says exactly where the range limit moved a value
    moved = ref['pre'] != ref['u8']
    bits = np.stack([(ref['mask'] >> c) & 1 for c in range(3)], -1).astype(bool)
    assert np.array_equal(bits, ~moved) and not (ref['mask'] >> 3).any()


@pytest.mark.parametrize('case', [c for c in S.CASES if c[2] == 'saturated'],
                         ids=[i for c, i in zip(S.CASES, S.CASE_IDS) if c[2] == 'saturated'])
def test_saturated_cases_clip_a_fair_share(case):
    share = S.clear_share(S.reference(*case)['mask'])
    print('clear share {:.3f}'.format(share))
    assert S.CLEAR_SHARE[0] <= share <= S.CLEAR_SHARE[1]


def test_unclipped_input_leaves_the_unit_interval_and_converts_per_value():
    for sub, shape in S.SHAPES:
        x = S.image(shape, 'unclipped')
        assert x.min() < 0 and x.max() > 1
        xb = S.convert(x)
        assert xb.min() == 0 and xb.max() == 255
        assert not np.array_equal(xb, jpeg_ref.to_bytes(x))             # the reference would have rescaled the whole batch


# ---- model surface ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['libjpeg+identity', 'libjpeg+sin', 'libjpeg+harmonic'])
def test_names_construct_and_describe_themselves(name):
    m = JPEG(75, name, device='cpu')
    assert repr(m) == 'JPEG(quality=75,codec="{}",trainable=False)'.format(name)
    assert m.summary() == 'JPEG ({}) QF=75'.format(name) == m.summary_compact()
    assert len(m.parameters) == 0
    m = JPEG(75, name, device='cpu', subsampling='4:2:0')
    assert repr(m) == 'JPEG(quality=75,codec="{}",trainable=False,subsampling="4:2:0")'.format(name)
    assert m.summary() == 'JPEG ({}) QF=75 4:2:0'.format(name)
    assert JPEG((50, 90), name, device='cpu').summary() == 'JPEG ({}) QF~[50,90]'.format(name)
    tables, clamped = JPEG(30, name, device='cpu').file_tables()        # libjpeg's own integer tables, nothing clamped
    assert tables.dtype == np.uint16 and not clamped.any()
    assert np.array_equal(tables, np.stack([jpeg_ref.qtable(30, 0), jpeg_ref.qtable(30, 1)]))


@pytest.mark.parametrize('name', ['libjpeg+sin', 'libjpeg+harmonic'])
def test_trainable_weights_start_as_the_differentiable_model_does(name):
    m, d = JPEG(60, name, trainable=True, device='cpu'), JPEG(60, name.split('+')[1], trainable=True, device='cpu')
    assert repr(m) == 'JPEG(quality=60,codec="{}",trainable=True)'.format(name)
    assert [tuple(p.shape) for p in m.parameters] == [(8, 8), (8, 8)]
    assert torch.equal(m._model.flat, d._model.flat)
    assert m.summary().startswith('JPEG ({}) trainable QF~'.format(name))


def test_refusals():
    with pytest.raises(ValueError, match='identically zero'):
        JPEG(60, 'libjpeg+identity', trainable=True, device='cpu')
    for name in ('libjpeg+identity', 'libjpeg+sin', 'libjpeg+harmonic'):
        with pytest.raises(ValueError, match='entropy_weight'):
            JPEG(60, name, device='cpu', entropy_weight=0.1)
    for name in ('libjpeg+soft', 'libjpeg+round', 'libjpeg+', '+sin'):
        with pytest.raises(ValueError, match='Unsupported codec version'):
            JPEG(60, name, device='cpu')
    with pytest.raises(ValueError, match='sub-sampling'):
        JPEG(60, 'libjpeg+sin', device='cpu', subsampling='4:1:1')
    with pytest.raises(ValueError, match='quality'):
        JPEG(None, 'libjpeg+sin', device='cpu').forward(torch.zeros(1, 8, 8, 3))


def test_existing_codecs_are_untouched():
    assert repr(JPEG(80, 'soft', device='cpu')) == 'JPEG(quality=80,codec="soft",trainable=False)'
    assert repr(JPEG(80, 'libjpeg', device='cpu')) == 'JPEG(quality=80,codec="libjpeg")'
    assert JPEG(80, 'soft', device='cpu').summary() == 'JPEG (soft) QF=80'
    assert JPEG(80, 'libjpeg', device='cpu').summary() == 'JPEG (libjpeg) QF=80'
    with pytest.raises(NotImplementedError):
        JPEG(80, 'libjpeg', device='cpu').forward(torch.zeros(1, 8, 8, 3), training=True)
    with pytest.raises(NotImplementedError):
        JPEG(80, 'libjpeg', device='cpu').backward({}, torch.zeros(1, 8, 8, 3))


# ---- ops.jpeg_ste_fwd: what is refused before a device is needed ---------------------------------------------------------------------
@pytest.mark.parametrize('shape, hs, vs', [((1, 8, 8), 1, 1), ((1, 12, 16, 3), 1, 1), ((1, 16, 12, 3), 1, 1), ((1, 8, 16, 3), 2, 2),
                                           ((1, 16, 8, 3), 2, 1), ((1, 16, 16, 4), 1, 1), ((1, 16, 16, 3), 1, 2), ((1, 16, 16, 3), 4, 1),
                                           ((1, 4104, 8, 3), 1, 1)])
def test_shape_refusals_need_no_device(shape, hs, vs):
    q = torch.ones((3, 64), dtype=torch.int16)
    with pytest.raises(ValueError):
        ops.jpeg_ste_fwd(torch.zeros(shape), q, hs, vs)


def test_argument_refusals_need_no_device():
    x = torch.zeros(1, 16, 16, 3)
    with pytest.raises(ValueError, match='output'):
        ops.jpeg_ste_fwd(x, torch.ones((3, 64), dtype=torch.int16), out=torch.zeros(1, 16, 16, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='output'):
        ops.jpeg_ste_fwd(x, torch.ones((3, 64), dtype=torch.int16), out=torch.zeros(1, 8, 16, 3))
    with pytest.raises(RuntimeError):                                   # no CPU path: a host tensor is refused, not computed
        ops.jpeg_ste_fwd(x, torch.ones((3, 64), dtype=torch.int16))
    assert ops.jpeg_ste_shape(torch.zeros(2, 48, 80, 3), 2, 2) == (2, 48, 80)
    assert ops.jpeg_ste_workspace_bytes(2, 48, 80, 2, 2) == 2 * 2 * 24 * 40
    assert ops.jpeg_ste_workspace_bytes(2, 24, 80, 2, 1) == 2 * 2 * 24 * 40
    assert ops.jpeg_ste_workspace_bytes(2, 48, 80, 1, 1) == 0
    assert ops.jpeg_ste_workspace_bytes(0, 48, 80, 2, 2) == 0           # empty
    assert ops.jpeg_ste_workspace_bytes(2, 40, 80, 2, 2) == 0           # ragged: refused
    assert ops.jpeg_ste_workspace_bytes(2, 48, 80, 1, 2) == 0           # other factors: refused
