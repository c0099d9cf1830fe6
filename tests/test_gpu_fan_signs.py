"""
Sign planes of the FAN's bf16-stored pooled activations (include/nimg.h): one bit per value, written by the
fused conv + pool kernels next to the activation, read by the next layer's input gradient INSTEAD of the activation for its
LeakyReLU' mask.  Nothing may change by a bit:

  producers   the plane equals (pooled bf16 value > 0) packed as specified (np.array_equal), pooled values and arg-max bytes are those
              of the call without the plane.  conv1_pool_fwd_kernel at both tile widths and a ragged shape; the ring pooling
              epilogue at the smallest batches that reach it (384 workgroups: 48 images for 128 channels, 96 for 64).  Whole
              images are zero, so every window sum there is exactly 0 and the pooled value is lrelu(bias): the biases make it
              +0, -0 (a negative float32 denormal times alpha), a negative and a POSITIVE value that round to -0 / +0 in bf16 - the
              bit is taken from the value as stored, not from the float32 one.
  consumers   conv2d_dgrad_unpool(act_mask, act_sign=plane) == conv2d_dgrad_unpool(act_mask) bit for bit at the shapes of the three
              ring forms, integer and full-mantissa operands, activations that carry +-0, denormals, infinities and NaNs.  An
              INVERTED plane must change the result where the kernel reads the plane (a child process with NIMG_TN32_BELOW=0: all
              three rings) and must not where the route cannot take it (this process: the 128- and 64-channel layers go to the
              32-channel tile below 384 workgroups and fall back to the mask silently).
  FAN         forward + backward at 2 x 64 x 64 with and without NIMG_NO_ACT_SIGN (child processes: ops reads it once): identical
              probabilities, loss, input gradient and parameter gradients.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fan_signs_cases as S
from conv_cases import full_mantissa
from util import ternary

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DENORM = float(np.float32(1.4e-45))            # the smallest float32 denormal


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    return torch.device('cuda', 0)


def special_biases(cout, seed):
    """Biases (float32) of a layer whose first image is zero: the pooled value there is lrelu(bias) = bias (> 0) or 0.2 bias."""
    b = ternary((cout,), seed, p=0.5)
    b[0:8] = [0.0, -0.0, -DENORM, DENORM, -1e-40, 1e-41, -3.0, 2.0]      # +0 | +0 | -0 | f32 > 0, bf16 +0 | -0 (bf16) | +0 (bf16) | < 0 | > 0
    return b


def check_plane(pooled, plane, what):
    pb = S.bits(pooled)
    assert plane.dtype == torch.uint8 and tuple(plane.shape) == tuple(pooled.shape[:3]) + (pooled.shape[3] // 8,), what
    assert np.array_equal(plane.cpu().numpy(), S.pack_signs(pb)), what + ': the plane is not (pooled > 0)'
    u = pb.view(np.uint16)
    assert (u == 0x0000).any() and (u == 0x8000).any(), what + ': the case plants no +0 / -0'
    v = S.bf16_value(pb)
    assert (v > 0).any() and (v < 0).any(), what


@pytest.mark.parametrize('shape', [(1, 8, 64), (1, 8, 256), (2, 10, 72)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv1_pool_writes_the_plane(dev, shape):
    from neural_imaging_amd import ops
    n, h, w = shape
    x = full_mantissa((n, h, w, 3), 41)
    x[0, :, : w // 2] = 0.0                              # windows whose sums are exactly 0
    c4 = torch.ones((n, h, w, 4), dtype=BF, device=dev)
    c4[..., :3] = torch.from_numpy(x).to(dev).to(BF)
    c4 = c4.contiguous()
    wt = torch.from_numpy(0.2 * full_mantissa((5, 5, 3, 32), 42)).to(dev)
    b = torch.from_numpy(special_biases(32, 43)).to(dev)
    ops.set_compute('bf16')
    assert ops.ACT_SIGN
    pooled0, idx0 = ops.conv1_pool_c4(c4, wt, b)
    pooled, idx, plane = ops.conv1_pool_c4(c4, wt, b, want_sign=True)
    torch.cuda.synchronize()
    assert np.array_equal(S.bits(pooled), S.bits(pooled0)) and torch.equal(idx, idx0)
    check_plane(pooled, plane, 'conv1_pool_c4 {}'.format(shape))
    # float32 storage has no plane
    assert ops.conv1_pool_c4(c4, wt, b, out_bf16=False, want_sign=True)[2] is None


@pytest.mark.parametrize('shape', [(48, 32, 32, 32, 128), (96, 32, 32, 32, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_ring_pool_writes_the_plane(dev, shape):
    from neural_imaging_amd import ops
    n, h, w, cin, cout = shape
    x = ternary((n, h, w, cin), 51)
    x[0] = 0.0
    xd = torch.from_numpy(x).to(dev).to(BF)
    wt = torch.from_numpy(ternary((5, 5, cin, cout), 52)).to(dev)
    b = torch.from_numpy(special_biases(cout, 53)).to(dev)
    ops.set_compute('bf16')
    assert ops.conv2d_pool_sign_ok(xd, wt), 'the shape does not reach a ring kernel'
    pooled0, idx0 = ops.conv2d_pool(xd, wt, b, out_bf16=True)
    pooled, idx, plane = ops.conv2d_pool(xd, wt, b, out_bf16=True, want_sign=True)
    torch.cuda.synchronize()
    assert plane is not None
    assert np.array_equal(S.bits(pooled), S.bits(pooled0)) and torch.equal(idx, idx0)
    check_plane(pooled, plane, 'conv2d_pool {}'.format(shape))


def test_pool_routes_without_a_plane_say_so(dev):
    """Below 384 workgroups the layer goes to the 32-channel tile, float32 storage has no bf16 value to take the bit from: the plane
    is None, pooled values and arg-max bytes are returned as ever; the entry point itself refuses to pretend (NIMG_ERR_ARG)."""
    from neural_imaging_amd import ops
    xd = torch.from_numpy(ternary((2, 32, 32, 32), 61)).to(dev).to(BF)
    wt = torch.from_numpy(ternary((5, 5, 32, 128), 62)).to(dev)
    ops.set_compute('bf16')
    assert not ops.conv2d_pool_sign_ok(xd, wt)
    pooled, idx, plane = ops.conv2d_pool(xd, wt, None, out_bf16=True, want_sign=True)
    pooled0, idx0 = ops.conv2d_pool(xd, wt, None, out_bf16=True)
    assert plane is None and torch.equal(pooled, pooled0) and torch.equal(idx, idx0)
    assert ops.conv2d_pool(xd, wt, None, out_bf16=False, want_sign=True)[2] is None
    junk = torch.empty((2, 16, 16, 16), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='NIMG_ERR_ARG'):
        ops._lib.call('nimg_conv2d_pool_fwd_bf16_sign', ops._p(xd), 32, ops._p(wt), ops._p(ops.weights_bf16(wt, 0)), None, ops._p(pooled),
                      ops._p(idx), ops._p(junk), 128, 2, 32, 32, 5, 1, 0.2, ops.BF16_IN | ops.BF16_OUT, ops._stream())


# ---- consumers ---------------------------------------------------------------------------------------------------------------
def faulted(returncode, stderr):
    """Did a child end the way a GPU fault ends one?  (as tests/test_gpu_conv_switches.py: no further GPU work after that)"""
    return returncode < 0 or returncode in (134, 139, 124, 137) or 'illegal memory access' in stderr or 'Memory access fault' in stderr


def run_child(mode, out, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith('NIMG_')}
    env.update(env_extra)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fan_signs_child.py')
    try:
        p = subprocess.run([sys.executable, child, mode, str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit('child {} {} ran into its time limit'.format(mode, env_extra), returncode=1)
    err = p.stderr.decode(errors='replace')
    if faulted(p.returncode, err):
        pytest.exit('child {} {} ended like a GPU fault ({}): {}'.format(mode, env_extra, p.returncode, err[-2000:]), returncode=1)
    assert p.returncode == 0, 'child {} failed ({}): {}'.format(mode, p.returncode, err[-3000:])
    with np.load(str(out)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def ring_consumers(dev, tmp_path_factory):
    return run_child('consumers', tmp_path_factory.mktemp('signs') / 'consumers.npz', {'NIMG_TN32_BELOW': '0'})


@pytest.mark.parametrize('kind', S.OPERAND_KINDS)
@pytest.mark.parametrize('shape', S.CONSUMER_SHAPES, ids=lambda s: '{}from{}'.format(s[3], s[4]))
def test_ring_dgrad_reads_the_plane(ring_consumers, shape, kind):
    name = S.consumer_name(shape, kind)
    mask, sign, inverted = (ring_consumers[name + '/' + k] for k in ('mask', 'sign', 'inverted'))
    assert mask.shape == (shape[0], shape[1], shape[2], shape[3]) and np.abs(S.bf16_value(mask)).max() > 0
    assert np.array_equal(sign, mask), name + ': the plane and the mask give different bits'
    assert not np.array_equal(inverted, mask), name + ': the kernel did not read the plane'


@pytest.mark.parametrize('shape', S.CONSUMER_SHAPES, ids=lambda s: '{}from{}'.format(s[3], s[4]))
def test_dgrad_routes_in_this_process(dev, shape):
    """The default dispatch at two images: 32 output channels run on conv5_ring_kernel<32, true> and read the plane; 128 and 64 go to
    the 32-channel tile (fewer than 384 workgroups), which cannot - it must use the mask it is handed with the plane, silently."""
    from neural_imaging_amd import ops
    o = S.consumer_operands(shape, 'full')
    g = torch.from_numpy(o['gp']).to(dev).to(BF)
    idx, w = torch.from_numpy(o['idx']).to(dev), torch.from_numpy(o['w']).to(dev)
    act = torch.from_numpy(o['act_bits']).to(dev).view(BF)
    plane = torch.from_numpy(S.pack_signs(o['act_bits'])).to(dev)
    ops.set_compute('bf16')
    mask = S.bits(ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True))
    sign = S.bits(ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True, act_sign=plane))
    inverted = S.bits(ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True, act_sign=~plane))
    f32out = ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=False, act_sign=~plane)         # float32 output: the mask
    assert np.array_equal(sign, mask)
    assert np.array_equal(inverted, mask) == (shape[3] != 32)
    assert torch.equal(f32out, ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=False))
    with pytest.raises(ValueError):                                                 # a plane without its mask, or of another shape
        ops.conv2d_dgrad_unpool(g, idx, w, out_bf16=True, act_sign=plane)
    with pytest.raises(ValueError):
        ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True, act_sign=plane[:, :, :, :-1].contiguous())


# ---- the FAN -----------------------------------------------------------------------------------------------------------------
def test_fan_gradients_do_not_change(dev, tmp_path):
    on = run_child('fan', tmp_path / 'on.npz', {})
    off = run_child('fan', tmp_path / 'off.npz', {'NIMG_NO_ACT_SIGN': '1'})
    assert list(on['planes']) == [1] and list(off['planes']) == [], (on['planes'], off['planes'])     # conv1's (conv2 .. 4: tiles at n = 2)
    assert sorted(on) == sorted(off) and any(k.startswith('grad/conv2/') for k in on)
    for k in on:
        if k != 'planes':
            assert np.array_equal(on[k], off[k], equal_nan=True), k
    assert np.isfinite(on['loss']).all() and np.abs(on['dx']).max() > 0
