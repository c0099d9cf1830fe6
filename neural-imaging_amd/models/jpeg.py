"""
JPEG compression models on the fused HIP kernel.  Mirrors the reference's models/jpeg.py:

  DifferentiableJPEG (:45-159)  - the codec itself; here one fused kernel per direction (nimg_djpeg_fwd/_bwd)
  JPEG (:162-286)               - framework wrapper: quality resolution/randomisation, codec switch
  differentiable_jpeg (:38-42)  - lazily created shared instance used by the 'jpeg' manipulation

Differences by design: Q tables are passed to the kernel per call, so the temporary table swap of JPEG.process
(:235-243, not re-entrant in the reference) has no shared state here.  The 'libjpeg' codec (:227-233) - the reference's
final-validation codec, a host round trip through imageio there - is the baseline codec of csrc/jpegc.hip here: libjpeg's
files and decoded images bit for bit, on the device (compression/jpeg_helpers.py).  It has no gradient.
New: JPEG.file_tables / JPEG.process_files run that real codec with the model's own tables - the learned ones, or those the
differentiable codec divides by - so the two stand side by side at identical tables.
New: subsampling='4:2:2' / '4:2:0' - the differentiable codec with the real codec's chroma sub-sampling (box down-sampling,
libjpeg's triangle up-sampling; csrc/djpeg_sub.hip).  '4:4:4' (the default) is the reference's model.
New: entropy_weight=w - the rate term the reference left commented out (:245-249, "takes too much memory"): the soft entropy of the
quantised DCT coefficients (csrc/djpeg_entropy.hip), reported by process(return_entropy=True) and added to the
gradients by backward(entropy_coef=).  None (the default) is the reference's model: the entropy is NaN and nothing else changes.
New: codec='libjpeg+identity' / 'libjpeg+sin' / 'libjpeg+harmonic' - a straight-through estimator of the real codec (csrc/jpeg_ste.hip,
DESIGN.md section 4o): the forward pass IS the real codec (the image libjpeg decodes from the file it would write, bit for bit, plus
the clip mask), the backward pass the differentiable codec's adjoint at the same input with the rounding surrogate named after '+'
('soft' has 'sin's backward and gets no name).  Fixed quality: libjpeg's own integer tables in both directions.  trainable=True: the
float weights of the differentiable model; the forward runs at their file_tables() rounding, the backward at the weights themselves.
"""
import numpy as np
import torch

from .. import ops
from ..device import DeviceArray, default_device, to_device
from ..helpers.utils import is_number
from ..compression.jpeg_helpers import compress_batch, device_codec, encode_batch, jpeg_qf_estimation, libjpeg_qtable
from .tfmodel import ParamStore, TFModel

_common_codec = None

# codec name -> rounding surrogate of the backward pass: the real codec forward, that surrogate's adjoint backward
STE_CODECS = {'libjpeg+identity': 'identity', 'libjpeg+sin': 'sin', 'libjpeg+harmonic': 'harmonic'}


def is_valid_quality(quality):
    if is_number(quality) and 1 <= quality <= 100:
        return True
    elif hasattr(quality, '__getitem__') and len(quality) > 1 and all((1 <= x <= 100) for x in quality):
        return True
    return False


def differentiable_jpeg(x, quality):
    global _common_codec
    if _common_codec is None:
        _common_codec = JPEG(None, 'soft')
    return _common_codec.process(x, quality)


class DifferentiableJPEG(object):
    """Holds the codec settings; __call__ returns (y, X_dequantised) like the Keras model's call()."""

    def __init__(self, quality=None, rounding_approximation='sin', rounding_approximation_steps=5, trainable=False,
                 device=None, subsampling='4:4:4'):
        self.subsampling = subsampling
        self.factors = ops.jpeg_subsampling(subsampling)          # ValueError for anything but 4:4:4, 4:2:2, 4:2:0
        if quality is not None and not is_valid_quality(quality):
            raise ValueError('Invalid JPEG quality: requires int in [1,100] or an iterable with least 2 such numbers')
        if rounding_approximation is not None and rounding_approximation not in ['sin', 'harmonic', 'soft']:
            raise ValueError('Unsupported rounding approximation: {}'.format(rounding_approximation))
        self.quality = quality
        self.trainable = trainable
        self.rounding_approximation = rounding_approximation
        self.rounding_approximation_steps = rounding_approximation_steps
        self.device = device
        self._q_cache = {}
        # trainable=True (models/jpeg.py:57-62): two (8,8) weights 'Q_mtx_luma' / 'Q_mtx_chroma', initialised from the IJG tables
        # of a numeric quality or ones; the chroma table serves Cb and Cr (:125-128).  Both sit back to back in ONE flat buffer
        # (64 floats each = the ParamStore's alignment), which is also the (2,8,8) layout nimg_djpeg_bwd_dq writes.
        self.params = None
        if trainable:
            self.params = ParamStore([('Q_mtx_luma', (8, 8)), ('Q_mtx_chroma', (8, 8))],
                                     device if device is not None else default_device())
            init = ops.qtables_device(quality if is_number(quality) else None, 'cpu')
            self.params.p['Q_mtx_luma'].copy_(init[0])
            self.params.p['Q_mtx_chroma'].copy_(init[1])

    def qtables(self, quality, device):
        key = (quality if is_number(quality) else None, str(device))
        if key not in self._q_cache:
            self._q_cache[key] = ops.qtables_device(key[0], device)
        return self._q_cache[key]

    def trainable_tables(self):
        """(3,8,8) [Y, Cb, Cr] view of the trainable weights for the kernel (one small gather per forward pass)."""
        return self.params.flat.view(2, 8, 8)[[0, 1, 1]].contiguous()

    def __call__(self, x, quality=None):
        q = self.trainable_tables() if (self.trainable and (quality is None or quality == self.quality)) else \
            self.qtables(self.quality if quality is None else quality, x.device)
        if self.factors != (1, 1):         # xdq: (X_luma (n,h/8,w/8,8,8), X_chroma (n,2,h/(8 vs),w/(8 hs),8,8))
            y, _, _, xdq = ops.djpeg_sub_fwd(x, q, self.rounding_approximation, *self.factors, want_mask=False, want_xdq=True)
            return y, xdq
        y, _, _, xdq = ops.djpeg_fwd(x, q, self.rounding_approximation, want_mask=False, want_xdq=True)
        return y, xdq


class JPEG(TFModel):

    def __init__(self, quality=None, codec='soft', trainable=False, device=None, subsampling='4:4:4', entropy_weight=None):
        super().__init__(device=device)
        if codec is not None and codec not in ['libjpeg', 'soft', 'sin', 'harmonic'] and codec not in STE_CODECS:
            raise ValueError('Unsupported codec version: {}'.format(codec))
        self._ste = STE_CODECS.get(codec)        # the backward surrogate of a real-codec forward, None for every other codec
        if self._ste is not None:
            if entropy_weight is not None:
                raise ValueError('entropy_weight: the rate of a real codec is its bytes, which process_files reports - codec "{}" has '
                                 'no soft rate term'.format(codec))
            if trainable and self._ste == 'identity':
                raise ValueError('codec "libjpeg+identity" with trainable=True: the table gradient of the identity surrogate is '
                                 'identically zero - train the tables through "libjpeg+sin" or "libjpeg+harmonic"')
        if entropy_weight is not None:
            if isinstance(entropy_weight, bool) or not is_number(entropy_weight) or not entropy_weight >= 0:
                raise ValueError('entropy_weight: None or a number >= 0 expected, got {!r}'.format(entropy_weight))
            if codec == 'libjpeg':
                raise ValueError('entropy_weight needs a differentiable codec: the libjpeg codec has no gradient, and its rate is '
                                 'real bytes (compression/jpeg_helpers.py)')
            if ops.jpeg_subsampling(subsampling) != (1, 1):
                raise ValueError('entropy_weight: the rate term covers the 4:4:4 codec only, got subsampling="{}"'.format(subsampling))
        self.entropy_weight = None if entropy_weight is None else float(entropy_weight)
        self._entropy_ws = {}                    # (shape, device) -> workspace: allocated once, re-used by every step
        self.subsampling = subsampling
        self._factors = ops.jpeg_subsampling(subsampling)         # ValueError for anything but 4:4:4, 4:2:2, 4:2:0
        # (the codec model of a straight-through codec only holds the trainable weights, initialised as the differentiable model's)
        approx = codec if self._ste is None else (None if self._ste == 'identity' else self._ste)
        self._codec_model = None if codec == 'libjpeg' else DifferentiableJPEG(quality, approx, trainable=trainable,
                                                                               device=self.device, subsampling=subsampling)
        self._rounding = codec if self._ste is None else self._ste          # what the kernels are told
        self._ste_cache = {}                     # (quality, device) -> (uint16 tables of the forward, float32 tables of the backward)
        # no trainable parameters unless trainable=True: then the two quantisation tables (models/jpeg.py:57-62)
        self._model = self._codec_model.params if (trainable and self._codec_model is not None) else ParamStore([], self.device)
        self.trainable = bool(trainable)
        self.codec = codec
        self.quality = quality
        self.loss = self._mse

    def _mse(self, y_true, y_pred, sample_weight=None):
        """tf.keras.losses.MeanSquaredError (models/jpeg.py:197). The workflow passes entropy = NaN as sample_weight
        (workflows/...:269); it is ignored here so the NaN does not propagate."""
        a, b = to_device(y_true, self.device), to_device(y_pred, self.device)
        return float(DeviceArray(ops.mse255(a, b)[0])) / (255.0 * 255.0)

    def reset_performance_stats(self):
        self.performance = self._reset_performance(['entropy', 'ssim', 'psnr'])

    @staticmethod
    def resolve_quality(quality):
        """Quality resolution of JPEG.process (models/jpeg.py:210-225)."""
        if not is_valid_quality(quality):
            raise ValueError('Invalid or unspecified JPEG quality!')
        if hasattr(quality, '__getitem__') and len(quality) > 2:
            return int(np.random.choice(quality))
        elif hasattr(quality, '__getitem__') and len(quality) == 2:
            return int(np.random.randint(quality[0], quality[1]))
        elif is_number(quality) and 1 <= quality <= 100:
            return int(quality)
        raise ValueError('Invalid quality! {}'.format(quality))

    # forward/backward used by the workflow ----------------------------------------------------------------------
    def forward(self, x, quality=None, training=False, out=None):
        if x.dim() == 4 and x.shape[3] == 1:
            raise ValueError('the JPEG model takes (n,h,w,3) batches: grey-scale (one-component) images are coded by '
                             'compression.jpeg_helpers alone (DESIGN.md section 4p)')
        if self._codec_model is None:
            if training:
                raise NotImplementedError('the libjpeg codec has no gradient (the reference has none either): train on a '
                                          'differentiable codec, validate on this one')
            # models/jpeg.py:227-233: compress_batch(batch_x, quality)[0], at the model's sub-sampling (4:4:4 there); the byte counts are not asked for here
            y, _ = device_codec(x, self.resolve_quality(self.quality if quality is None else quality), self.subsampling,
                                want_bytes=False)
            if out is not None:
                out.copy_(y)
                y = out
            return y, None
        # the quality is resolved FIRST (an invalid / unspecified one raises even with trainable tables); the model's own tables -
        # the learned ones - serve iff the resolved quality is the constructor's, any other quality swaps in its IJG tables for
        # this call (models/jpeg.py:210-243)
        resolved = self.resolve_quality(self.quality if quality is None else quality)
        learned = bool(self.trainable) and is_number(self.quality) and resolved == self.quality
        if self._ste is not None:
            return self._forward_ste(x, resolved, learned, training, out)
        if learned:
            q = self._codec_model.trainable_tables()
        else:
            q = self._codec_model.qtables(resolved, x.device)
        if self._factors != (1, 1):
            y, mask, _, _ = ops.djpeg_sub_fwd(x, q, self.codec, *self._factors, want_mask=training, out=out)
        else:
            y, mask, _, _ = ops.djpeg_fwd(x, q, self.codec, want_mask=training, out=out)
        if not training:
            return y, None
        ctx = {'x': x, 'mask': mask, 'q': q, 'learned': learned}
        if self.entropy_weight is not None:
            ctx['entropy'], ctx['entropy_ws'] = self._entropy(x, q)
        return y, ctx

    def _ste_tables(self, quality, device):
        """libjpeg's own integer tables of a quality on the device, for both directions of a straight-through codec: ((1,3,64) int16
        holding the uint16 entries for the forward, (3,8,8) float32 for the backward)."""
        key = (int(quality), str(device))
        if key not in self._ste_cache:
            t = np.stack([libjpeg_qtable(quality, c).ravel() for c in (0, 1, 1)])
            self._ste_cache[key] = (torch.from_numpy(t.astype(np.int16).reshape(1, 3, 64)).to(device),
                                    torch.from_numpy(t.astype(np.float32).reshape(3, 8, 8)).to(device))
        return self._ste_cache[key]

    def _forward_ste(self, x, resolved, learned, training, out):
        """The real codec forward (ops.jpeg_ste_fwd).  Learned tables: the file_tables() rule on the device (ops.jpeg_tables_from_float),
        no status read in the step; the backward differentiates at the float weights."""
        if learned:
            q = self._codec_model.trainable_tables()
            qtabs, _ = ops.jpeg_tables_from_float(q.view(1, 3, 64))
        else:
            qtabs, q = self._ste_tables(resolved, x.device)
        y, mask, _ = ops.jpeg_ste_fwd(x, qtabs, *self._factors, want_mask=training, out=out)
        if not training:
            return y, None
        return y, {'x': x, 'mask': mask, 'q': q, 'learned': learned}

    def _entropy(self, x, q):
        """(entropy (1,) on the device, workspace) of the batch x at the tables q.  The workspace belongs to the model and serves
        every call on the same shape (no per-step allocation: a captured step replays); it holds what backward() needs until the
        next forward pass on that shape."""
        key = (tuple(x.shape), str(x.device))
        if key not in self._entropy_ws:
            self._entropy_ws[key] = ops.djpeg_entropy_workspace(x)
        return ops.djpeg_entropy_fwd(x, q, self.codec, ws=self._entropy_ws[key])

    def backward(self, ctx, dy, accumulate=False, entropy_coef=0.0):
        """d loss / d x; with trainable tables also fills (accumulate: adds to) their gradients in the model's gradient buffer.
        entropy_coef (a model with entropy_weight): adds entropy_coef * d H / d x to the returned gradient and, with learned tables,
        entropy_coef * d H / d Q to theirs."""
        gx = self._backward_distortion(ctx, dy, accumulate)
        if entropy_coef:
            if ctx.get('entropy_ws') is None:
                raise ValueError('entropy_coef needs a model with entropy_weight and the ctx of forward(training=True)')
            ops.djpeg_entropy_bwd(ctx['x'], ctx['q'], ctx['entropy_ws'], entropy_coef, self.codec, out=gx, accumulate=True,
                                  dq=self._model.flat_grad if ctx.get('learned') else None, accumulate_dq=True)
        return gx

    def _backward_distortion(self, ctx, dy, accumulate):
        if self._codec_model is None:
            raise NotImplementedError('the libjpeg codec has no gradient')
        if self._factors != (1, 1):
            if ctx.get('learned'):
                return ops.djpeg_sub_bwd(ctx['x'], dy, ctx['mask'], ctx['q'], self._rounding, *self._factors,
                                         dq=self._model.flat_grad, accumulate=accumulate)
            return ops.djpeg_sub_bwd(ctx['x'], dy, ctx['mask'], ctx['q'], self._rounding, *self._factors)
        if ctx.get('learned'):
            return ops.djpeg_bwd(ctx['x'], dy, ctx['mask'], ctx['q'], self._rounding, dq=self._model.flat_grad, accumulate=accumulate)
        return ops.djpeg_bwd(ctx['x'], dy, ctx['mask'], ctx['q'], self._rounding)

    def process(self, batch_x, quality=None, return_entropy=False):
        """Compress a batch (NHW3 rgb): number -> that quality; 2 numbers -> random integer in [lo, hi);
        more -> random choice (models/jpeg.py:202-251).  Entropy is NaN, as in the reference (:245-249) - unless the model has an
        entropy_weight: then the soft entropy of the quantised DCT coefficients at the tables this call used."""
        x = to_device(batch_x, self.device)
        if self.entropy_weight is None or not return_entropy:
            y, _ = self.forward(x, quality)
            y = DeviceArray(y)
            return (y, np.nan) if return_entropy else y
        y, ctx = self.forward(x, quality, training=True)          # the ctx carries the tables the (possibly random) quality chose
        return DeviceArray(y), float(ctx['entropy'][0])

    # the real codec with the model's own tables ---------------------------------------------------
    def file_tables(self):
        """The model's own (luma, chroma) tables as a baseline file can carry them: (tables (2, 64) uint16 in natural order, clamped
        (2, 64) bool).  The learned weights with trainable=True, else the tables of the constructor's quality as the differentiable
        codec uses them (_model_tables), rounded to the nearest integer (ties to even) and clamped to 1..255 on the device
        (ops.jpeg_tables_from_float); `clamped` marks the entries that rule had to move - below 1, above 255 or not finite.
        codec='libjpeg': libjpeg's own tables of the numeric quality, nothing clamped."""
        if self._codec_model is None:
            if not is_number(self.quality):
                raise ValueError('file_tables needs a numeric quality with codec="libjpeg", got {}'.format(self.quality))
            q = self.resolve_quality(self.quality)
            return np.stack([libjpeg_qtable(q, c).ravel() for c in (0, 1)]).astype(np.uint16), np.zeros((2, 64), bool)
        if self._ste is not None and not self.trainable:           # a straight-through codec divides by libjpeg's own tables
            if not is_number(self.quality):
                raise ValueError('file_tables needs a numeric quality with codec="{}", got {}'.format(self.codec, self.quality))
            q = self.resolve_quality(self.quality)
            return np.stack([libjpeg_qtable(q, c).ravel() for c in (0, 1)]).astype(np.uint16), np.zeros((2, 64), bool)
        if self.trainable:
            t = self._codec_model.params.flat.detach().view(1, 2, 64)
        else:
            t = self._codec_model.qtables(self.quality, self.device)[:2].reshape(1, 2, 64)
        t = t.contiguous()
        qtabs, _ = ops.jpeg_tables_from_float(t)
        both = torch.cat([qtabs[0, :2].reshape(-1).float(), t.reshape(-1)]).cpu().numpy()          # one download
        tables, t = both[:128].reshape(2, 64).astype(np.uint16), both[128:].reshape(2, 64)
        with np.errstate(invalid='ignore'):
            return tables, ~np.isfinite(t) | (np.rint(t) < 1) | (np.rint(t) > 255)

    def process_files(self, batch_x, subsampling=None, optimize=False, return_files=False):
        """The real codec with exactly file_tables(), at `subsampling` or (None) the model's own: (float32 (n,h,w,3) batch libjpeg
        decodes, list of byte counts[, list of the
        files]) - what the learned tables, or the soft / sin / harmonic codec's, cost in bytes and do to the image once a standard
        encoder holds them.  Forward only: the real codec has no gradient (forward(training=True) of the libjpeg codec says the same)."""
        x = to_device(batch_x, self.device)
        if tuple(x.shape)[-1:] == (1,):
            raise ValueError('process_files needs an (n,h,w,3) batch: grey-scale (one-component) images are coded by '
                             'compression.jpeg_helpers alone (DESIGN.md section 4p)')
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise NotImplementedError('the real codec has no gradient (the reference has none either): train on a differentiable '
                                      'codec, measure on this one')
        tables, _ = self.file_tables()
        if subsampling is None:
            subsampling = self.subsampling
        y, sizes = compress_batch(x, None, subsampling=subsampling, optimize=optimize, qtables=tables)
        if y.ndim == 3:
            raise ValueError('process_files needs an (n,h,w,3) batch')
        if return_files:
            # x is float32 here, so the files hold the bytes compress_batch coded: the reference's conversion, no uint8 short cut
            return y, sizes, encode_batch(x, None, subsampling, optimize=optimize, qtables=tables)
        return y, sizes

    def __repr__(self):
        sub = '' if self._factors == (1, 1) else ',subsampling="{}"'.format(self.subsampling)
        if self._codec_model is not None:              # models/jpeg.py:253-257
            ew = '' if self.entropy_weight is None else ',entropy_weight={}'.format(self.entropy_weight)
            return 'JPEG(quality={},codec="{}",trainable={}{}{})'.format(self.quality, self.codec, bool(self.trainable), sub, ew)
        return 'JPEG(quality={},codec="{}"{})'.format(self.quality, self.codec, sub)

    def _sub_suffix(self):
        sub = '' if self._factors == (1, 1) else ' ' + self.subsampling
        return sub if self.entropy_weight is None else '{} H+{}'.format(sub, self.entropy_weight)

    def summary(self, quality=None):
        return 'JPEG ({}) {}{}'.format(self.codec, self._quality_mode(quality), self._sub_suffix())

    def summary_compact(self, quality=None):
        return 'JPEG ({}) {}{}'.format(self.codec, self._quality_mode(quality), self._sub_suffix())

    def _model_tables(self):
        """The codec model's own (luma, chroma) tables on the host: the learned weights with trainable=True, else the IJG tables of
        a numeric constructor quality, else ones (models/jpeg.py:57-66)."""
        if self.trainable:
            t = self._codec_model.params.flat.detach().cpu().view(2, 8, 8).numpy()
            return t[0], t[1]
        q = self._codec_model.qtables(self.quality, torch.device('cpu')).numpy()
        return q[0], q[1]

    def estimate_qf(self, channel=0):
        """Closest IJG quality of the current tables.  Like the reference (models/jpeg.py:265-269) the LUMA table is compared
        whatever `channel` says - `channel` only picks the IJG family it is compared with."""
        return jpeg_qf_estimation(self._model_tables()[0], channel)

    def _quality_mode(self, quality=None):
        quality = quality or self.quality
        if self.trainable and self._codec_model is not None:           # models/jpeg.py:274-278
            luma, chroma = self._model_tables()
            return 'trainable QF~{}/{}'.format(jpeg_qf_estimation(luma, 0), jpeg_qf_estimation(chroma, 1))
        elif is_number(quality):
            return 'QF={}'.format(quality)
        elif hasattr(quality, '__getitem__') and len(quality) == 2:
            return 'QF~[{},{}]'.format(*quality)
        elif hasattr(quality, '__getitem__') and len(quality) > 2:
            return 'QF~{{{}}}'.format(','.join(str(x) for x in quality))
        return 'QF=?'
