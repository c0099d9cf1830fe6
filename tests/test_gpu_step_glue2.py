"""
The short launches taken off the training step's critical path ("step glue"), each against the launches it
replaces, byte for byte:

  adam_images_kernel            adam_images-* : ParamStore.adam in throughput mode = ops.adam_step on a copy + WeightImages.refresh()
                                on the updated copy (p, m, v, both images of every 4-D weight); host rate and device rate,
                                grad_scale != 1, skip_flag 0 / 1 (a skipped update writes nothing, images included)
  ... its constrained-kernel workgroup   constrained-strength{1,100}: the store's normalised filter and flipped form =
                                ops.constrained_kernel / ops.flip_weights on the updated kernel; made again after a write
  the validity rule          images_current_*: refresh_images() launches nothing after a training step, rebuilds after a torch
                                write through a parameter view and after a change of the compute mode (device and host test)
  cdgrad_border_strip_kernel    border-*: nimg_cconv3_dgrad_border_strips = nimg_cconv3_dgrad_border on dyadic data, += onto a
                                non-zero dx; 4x4 (every pixel mirrors twice), one unit per side, several units per side
  whole step                    the C4 workflow at raw patch 16, B = 2, three steps with the switches off and on, eager and
                                captured, also with a weight written in place between steps 2 and 3
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from util import bayer_from_rgb, natural_images


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    return torch.device('cuda', 0)


# 3x3x5x7: padding in both images; 3x3x64x80: a whole 64 x 64 block and a partial one; 7x5 and the biases: the plain loop between
# the weights; every parameter starts on a 64-element boundary, the total is 195.25 x 256
SPECS = [('a/kernel', (3, 3, 5, 7)), ('a/bias', (7,)), ('b/kernel', (1, 1, 16, 64)), ('c/kernel', (2, 2, 32, 16)),
         ('d/kernel', (5, 5, 3, 3)), ('e/kernel', (3, 3, 64, 80)), ('f/kernel', (7, 5)), ('g/bias', (3,)), ('h/bias', (3,))]


def _filled_store(dev, seed):
    from neural_imaging_amd.models.tfmodel import ParamStore
    store = ParamStore(OrderedDict(SPECS), dev)
    gen = torch.Generator().manual_seed(seed)
    n = store.flat.numel()
    assert n % 256 != 0
    store.flat.copy_(torch.randn(n, generator=gen) * 0.1)
    store.flat_grad.copy_(torch.randn(n, generator=gen) * 0.01)
    store.ensure_adam()
    store.m.copy_(torch.randn(n, generator=gen) * 0.01)
    store.v.copy_(torch.rand(n, generator=gen) * 1e-4)
    return store


def _images(store):
    from neural_imaging_amd import ops
    return [ops.weights_bf16(w, mode).clone() for w, mode in store.images.entries]


@pytest.mark.gpu
@pytest.mark.parametrize('rate,gscale,flag', [('host', 1.0, None), ('host', 0.5, 0), ('dev', 0.25, 0), ('dev', 1.0, None),
                                              ('host', 0.5, 1), ('dev', 1.0, 1)],
                         ids=lambda v: str(v))
def test_adam_images_equals_adam_then_refresh(dev, rate, gscale, flag):
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    assert ops.ADAM_IMAGES
    fused, plain = _filled_store(dev, 5), _filled_store(dev, 5)
    assert len(fused.images.entries) == 10 and fused.images.within(fused.flat)
    before = [t.clone() for t in (fused.flat, fused.m, fused.v)]
    fused.refresh_images()                                     # the images of the weights before the update ...
    old_images = _images(fused)
    if flag != 1:
        fused.images.buf.fill_(0xAB)                           # ... which an update that is not skipped overwrites completely
    skip = None if flag is None else torch.full((1,), flag, dtype=torch.int32, device=dev)
    lr_t = None if rate == 'host' else torch.full((1,), ops.adam_lr_t(1e-3, 3), dtype=torch.float32, device=dev)
    fused.adam(1e-3, step=3, grad_scale=gscale, skip_flag=skip, lr_t_dev=lr_t)
    ops.adam_step(plain.flat, plain.flat_grad, plain.m, plain.v, 1e-3, 3, grad_scale=gscale, skip_flag=skip, lr_t_dev=lr_t)
    plain.images.refresh()
    for a, b in zip((fused.flat, fused.m, fused.v), (plain.flat, plain.m, plain.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for (w, mode), a, b in zip(fused.images.entries, _images(fused), _images(plain)):
        assert torch.equal(a, b), 'image mode {} of {}'.format(mode, tuple(w.shape))
    if flag == 1:
        for a, b in zip((fused.flat, fused.m, fused.v), before):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for a, b in zip(_images(fused), old_images):
            assert torch.equal(a, b)
    else:
        assert not torch.equal(fused.flat, before[0])
    assert fused.images_current()                              # (with a skip flag: because they were current before)


@pytest.mark.gpu
def test_adam_images_with_a_skip_flag_does_not_vouch_for_stale_images(dev):
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    store = _filled_store(dev, 6)
    store.refresh_images()
    store.p['e/kernel'].mul_(2)
    store.adam(1e-3, step=1, skip_flag=torch.ones(1, dtype=torch.int32, device=dev))
    assert not store.images_current()
    store.adam(1e-3, step=1)                                   # no flag: the launch always writes
    assert store.images_current()


@pytest.mark.gpu
@pytest.mark.parametrize('strength', [1.0, 100.0], ids=lambda v: 'strength{:g}'.format(v))
def test_adam_images_leaves_the_constrained_filter(dev, strength):
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    assert ops.ADAM_CCONV
    fused, plain = _filled_store(dev, 9), _filled_store(dev, 9)
    fused.register_constrained('d/kernel', strength)
    nf0 = fused.constrained_filter()[0].clone()                # today's two launches into the store's buffers
    assert fused.constrained_current()
    assert torch.equal(nf0, ops.constrained_kernel(plain.p['d/kernel'], strength))
    fused.refresh_images()
    fused.images.buf.fill_(0xAB)
    fused.constrained['nf'].fill_(7.0)
    fused.constrained['nft'].fill_(7.0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)       # (the workflow always passes its NaN flag)
    fused.adam(1e-3, step=2, grad_scale=0.5, skip_flag=flag)
    ops.adam_step(plain.flat, plain.flat_grad, plain.m, plain.v, 1e-3, 2, grad_scale=0.5, skip_flag=flag)
    plain.images.refresh()
    for a, b in zip((fused.flat, fused.m, fused.v), (plain.flat, plain.m, plain.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for (w, mode), a, b in zip(fused.images.entries, _images(fused), _images(plain)):
        assert torch.equal(a, b), 'image mode {} of {}'.format(mode, tuple(w.shape))
    nf = ops.constrained_kernel(plain.p['d/kernel'], strength)
    assert not torch.equal(nf, nf0) and bool(torch.isfinite(nf).all())
    assert fused.constrained_current()
    got_nf, got_flip = fused.constrained_filter()              # current: the buffers as the Adam launch left them
    assert got_nf is fused.constrained['nf'] and got_flip is fused.constrained['nft']
    assert torch.equal(got_nf.view(torch.int32), nf.view(torch.int32))
    assert torch.equal(got_flip.view(torch.int32), ops.flip_weights(nf).view(torch.int32))
    fused.p['d/kernel'].mul_(2)                                # a write: made again on demand
    assert not fused.constrained_current()
    nf2 = ops.constrained_kernel(fused.p['d/kernel'], strength)
    got_nf, got_flip = fused.constrained_filter()
    assert torch.equal(got_nf, nf2) and torch.equal(got_flip, ops.flip_weights(nf2)) and fused.constrained_current()
    fused.adam(1e-3, step=3, skip_flag=torch.ones(1, dtype=torch.int32, device=dev))       # skipped: nothing moves
    assert torch.equal(fused.constrained['nf'], nf2) and fused.constrained_current()


def test_images_current_rule_on_the_host():
    from neural_imaging_amd import ops
    from neural_imaging_amd.models.tfmodel import ParamStore
    store = ParamStore(OrderedDict(SPECS), 'cpu')
    ops.set_compute('bf16')
    assert not store.images_current()
    store._images_made = (store.flat._version, ops.COMPUTE_EPOCH)
    assert store.images_current()
    store.p['a/bias'].add_(1)                                  # any torch write through any view
    assert not store.images_current()
    store._images_made = (store.flat._version, ops.COMPUTE_EPOCH)
    ops.set_compute('bf16')                                    # no change of mode
    assert store.images_current()
    ops.set_compute('f32')
    assert not store.images_current()
    ops.set_compute('bf16')
    assert not store.images_current()
    store._images_made = (store.flat._version, ops.COMPUTE_EPOCH)
    store.invalidate_images()
    assert not store.images_current()


def _c4(dev):
    from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification
    dist = {'downsampling': 'none', 'compression': 'jpeg', 'compression_params': {'quality': 80, 'codec': 'soft'}}
    return ManipulationClassification('UNet', manipulations=['sharpen:1', 'resample:50', 'gaussian:0.83', 'jpeg:80'],
                                      distribution=dist, trainable={'nip'}, raw_patch_size=16, device=dev, nan_check='deferred')


def _batch(dev):
    rgb = natural_images(2, 32, 32, seed=77)
    return torch.from_numpy(bayer_from_rgb(rgb)).to(dev), torch.from_numpy(rgb).to(dev)


@pytest.mark.gpu
def test_images_current_after_a_training_step(dev):
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    wf = _c4(dev)
    bx, by = _batch(dev)
    wf.training_step(bx, by, lambda_nip=0.1, learning_rate=1e-4)
    for store in (wf.nip._model, wf.fan._model):
        good = store.images.buf.clone()
        store.images.buf.fill_(0xAB)
        store.refresh_images()                                 # nothing is launched: the poison stays
        assert bool((store.images.buf == 0xAB).all())
        store.images.buf.copy_(good)
    for store in (wf.nip._model, wf.fan._model):               # (the change of mode below reaches every model)
        name = next(k for k, t in store.p.items() if t.dim() == 4)
        store.p[name].mul_(2)
        assert not store.images_current()
        store.images.buf.fill_(0xAB)
        store.refresh_images()
        rebuilt = _images(store)
        store.images.buf.fill_(0)
        store.images.refresh()
        assert all(torch.equal(a, b) for a, b in zip(rebuilt, _images(store)))
        assert store.images_current()
        ops.set_compute('f32')
        ops.set_compute('bf16')
        store.images.buf.fill_(0xAB)
        store.refresh_images()
        assert all(torch.equal(a, b) for a, b in zip(rebuilt, _images(store)))
    wf.check_nan()


# ---- the mirror terms of the constrained filter's input gradient
@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(4, 4), (8, 16), (16, 64), (5, 7), (72, 136), (134, 66)], ids=lambda v: str(v))
def test_border_strips_equal_the_per_pixel_kernel(dev, h, w):
    from neural_imaging_amd import ops
    rng = np.random.RandomState(h * 1000 + w)
    dy = torch.from_numpy(rng.randint(-64, 65, (2, h, w, 3)).astype(np.float32) / 8).to(dev)
    nf = torch.from_numpy(rng.randint(-32, 33, (5, 5, 3, 3)).astype(np.float32) / 16).to(dev)
    dx0 = torch.from_numpy(rng.randint(-256, 257, (2, h, w, 3)).astype(np.float32) / 4).to(dev)
    old = ops.cconv3_dgrad_border(dy, nf, dx0.clone(), strips=False)
    new = ops.cconv3_dgrad_border(dy, nf, dx0.clone(), strips=True)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    touched = (old != dx0).any(dim=3)
    assert bool(touched[:, :2].any()) and bool(touched[:, -2:].any()) and not bool(touched[:, 2:-2, 2:-2].any())


# ---- the whole step
def _run_steps(dev, monkeypatch, on, captured, write):
    from neural_imaging_amd import graphs, ops
    for switch in ('ADAM_IMAGES', 'ADAM_CCONV', 'BORDER_STRIPS'):
        monkeypatch.setattr(ops, switch, on)
    wf = _c4(dev)
    bx, by = _batch(dev)
    kw = dict(lambda_nip=0.1, learning_rate=1e-3)
    losses = []
    if captured:
        runner = graphs.CapturedStep(wf, bx, by, warmup=1, **kw)          # (the warm-up step is step 1)
        step = lambda: runner.step()
    else:
        step = lambda: wf.training_step(bx, by, **kw)
        losses.append(float(step()[0]))
    losses.append(float(step()[0]))
    if write:
        name = next(k for k, t in wf.nip._model.p.items() if t.dim() == 4 and t.shape[2] >= 32)
        wf.nip._model.p[name].mul_(1.5)
    losses.append(float(step()[0]))
    wf.check_nan()
    assert wf._step == 3
    return losses, wf.nip._model.flat.clone(), wf.fan._model.flat.clone()


@pytest.mark.gpu
@pytest.mark.parametrize('captured', [False, True], ids=['eager', 'captured'])
@pytest.mark.parametrize('write', [False, True], ids=['', 'weight-written'])
def test_whole_step_is_unchanged_by_the_switches(dev, monkeypatch, captured, write):
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    off = _run_steps(dev, monkeypatch, False, captured, write)
    on = _run_steps(dev, monkeypatch, True, captured, write)
    assert off[0] == on[0] and all(np.isfinite(off[0]))
    assert torch.equal(off[1].view(torch.int32), on[1].view(torch.int32))
    assert torch.equal(off[2].view(torch.int32), on[2].view(torch.int32))
