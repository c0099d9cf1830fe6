"""
Image quality metrics on the device - the counterpart of the reference's helpers/metrics.py (ssim :9-25, psnr :28-44,
mse :47-65, mae :68-86, batch :89-92), which wraps skimage on host arrays.  Same call shapes: two (H,W,C) images return
a scalar, two (N,H,W,C) batches return one value per image; inputs may be numpy arrays or DeviceArrays.

msssim / msssim_db are new here: the columns of compression/ratedistortion.py.  msssim is tf.image.ssim_multiscale(a, b, 1.0), the
definition the reference trains with (helpers/tf_helpers.py:43-44); the reference's tables take theirs from sewar.full_ref.msssim,
and nothing here pins the two against each other.
"""
import warnings

import numpy as np
import torch

from .. import ops
from ..device import DeviceArray, default_device, to_device


def _pair(a, b):
    a = a.t if isinstance(a, DeviceArray) else a
    b = b.t if isinstance(b, DeviceArray) else b
    dev = a.device if isinstance(a, torch.Tensor) and a.is_cuda else (
        b.device if isinstance(b, torch.Tensor) and b.is_cuda else default_device())
    a, b = to_device(a, dev), to_device(b, dev)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    if b.ndim == 4 and b.shape[0] == 1:
        b = b[0]
    if a.ndim != b.ndim or a.ndim not in (3, 4):
        raise ValueError('Incompatible tensor shapes! {} and {}'.format(tuple(a.shape), tuple(b.shape)))
    single = a.ndim == 3
    if single:
        a, b = a[None], b[None]
    return a.contiguous(), b.contiguous(), single


def _ret(v, single):
    v = v.double().cpu().numpy()
    return float(v[0]) if single else v


def ssim(a, b):
    """skimage.metrics.structural_similarity(a, b, multichannel=True, data_range=1): 7x7 uniform window."""
    a, b, single = _pair(a, b)
    return _ret(ops.ssim(a, b, mode='skimage', max_val=1.0), single)


def _mean_per_image(a, b, fn):
    d = fn(a.double() - b.double())
    return d.reshape(d.shape[0], -1).mean(dim=1)


def mse(a, b):
    a, b, single = _pair(a, b)
    return _ret(_mean_per_image(a, b, lambda d: d * d), single)


def mae(a, b):
    a, b, single = _pair(a, b)
    return _ret(_mean_per_image(a, b, torch.abs), single)


def psnr(a, b):
    """skimage.metrics.peak_signal_noise_ratio(a, b, data_range=1) = 10 log10(1 / mse)."""
    a, b, single = _pair(a, b)
    return _ret(10.0 * torch.log10(1.0 / _mean_per_image(a, b, lambda d: d * d)), single)


_MSSSIM_WARNED = False


def msssim_ok(h, w):
    """The size rule of ops.msssim / ops.msssim_loss: multiples of 16 with h / 16 and w / 16 at least 11."""
    div = 1 << (ops.MSSSIM_SCALES - 1)
    return h % div == 0 and w % div == 0 and h // div >= 11 and w // div >= 11


def _msssim_device(a, b):
    """(n,) float64 device tensor of two device batches, or None - after the one warning - for sizes that break the rule."""
    global _MSSSIM_WARNED
    if msssim_ok(a.shape[1], a.shape[2]):
        return ops.msssim(a, b, max_val=1.0)
    if not _MSSSIM_WARNED:
        _MSSSIM_WARNED = True
        warnings.warn('MS-SSIM needs image sizes that are multiples of 16 and at least 176 pixels: nan for {} x {} images '
                      '(said once)'.format(a.shape[1], a.shape[2]))
    return None


def msssim(a, b):
    """tf.image.ssim_multiscale(a, b, max_val=1) per image.  Images that break the size rule (msssim_ok) give nan - one small image
    must not stop a table - and the module says so once."""
    a, b, single = _pair(a, b)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError('Incompatible tensor shapes! {} and {}'.format(tuple(a.shape), tuple(b.shape)))
    v = _msssim_device(a, b)
    if v is None:
        return float('nan') if single else np.full((a.shape[0],), np.nan)
    return _ret(v, single)


def msssim_db(a, b):
    """-10 log10(1 - msssim(a, b)), the reference's msssim_db column (inf for identical images)."""
    with np.errstate(divide='ignore'):
        return -10.0 * np.log10(1.0 - msssim(a, b))


def batch(a, b, metric=ssim):
    assert a.ndim == 4 and b.ndim == 4, 'Input arrays need to be 4-dim: batch, height, width, channels'
    assert len(a) == len(b), 'Image batches must be of the same length'
    return float(np.mean(metric(a, b)))
