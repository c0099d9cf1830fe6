"""
The l3ic bitstream of the learned codec (DCN / TwitterDCN): the reference's compression/codec.py with its names and call
shapes (compress :87-185, decompress :188-265, simulate_compression / compress_n_stats :19-52, restore), coded on the GPU.
The per-layer work - vector quantisation, entropy coding and decoding - runs in libnimg.so (nimg_l3ic_*), a whole batch of
(image, feature layer) streams per launch; compress_batch / decompress_batch code a batch with one host synchronisation.

Bit stream (all integers little-endian).  The container is the reference's byte for byte:

    container = shape[3] (uint8: latent H, W, N)
              | uint16 len_lengths (always 2N: the layer lengths are stored raw)
              | uint16 layer_length[N]
              | layer_payload[0] ... layer_payload[N-1]

Layer n holds z[0, :, :, n] in row-major (H, W) order as codebook indices, n_sym = H * W symbols.  The decoder tells the
payload kind by its length: == n_sym RAW (the index bytes), == 3 RLE (uint16 count, uint8 symbol), otherwise rANS.  The
encoder writes RLE when one symbol fills the layer, else rANS when that is strictly shorter than n_sym, else RAW; so the
decoder refuses a payload longer than n_sym.

The entropy-coded payload is interleaved rANS, not the reference's FSE (no FSE implementation could pin pyfse's bytes):

    uint8  L            lanes, 1..64; the encoder uses min(64, largest power of two <= max(1, n_sym // 2048))
    uint8  a, b         first and last symbol index with a non-zero frequency
    varint f[a..b]      normalised frequencies, unsigned LEB128 (<= 2 bytes each), summing to exactly 4096
    uint32 x[L]         final encoder states, lane 0 first
    uint16 words[...]   renormalisation words in decode order

Probability scale 4096, states in [2^16, 2^32), 16-bit words.  Symbol i belongs to lane i % L at step i // L.  Decoding
step by step from 0, every active lane takes slot = x & 4095, s = sym[slot], x = f[s] (x >> 12) + slot - cum[s], and a
lane left with x < 2^16 reads one word (x = x << 16 | word), lanes in ascending order from one word pointer.  A valid
stream uses every word and leaves every lane at 2^16.  Frequencies: f_s = max(1, c_s 4096 // n) for c_s > 0; a deficit
goes to the largest count, a surplus is taken 1 at a time from the largest f > 1 (ties to the lowest index).  DESIGN.md
"l3ic bitstream" has the whole contract.
"""
import json
import struct
from pathlib import Path

import numpy as np
import torch

from .. import ops
from ..device import DeviceArray, default_device, to_device
from ..helpers import metrics


class L3ICError(Exception):
    pass


# ---- container (host only) ------------------------------------------------------------------------------------------
def check_latent_shape(h, w, n, codebook_size):
    if codebook_size > 256:
        raise L3ICError('Code-books with more than 256 centers are not supported')
    if max(h, w, n) > 255:
        raise L3ICError('Latent shape {}x{}x{} does not fit the bitstream (at most 255 per axis)'.format(h, w, n))
    if h * w < 4:
        raise L3ICError('Latent layers of {} values are not supported (at least 4)'.format(h * w))


def pack_container(h, w, payloads):
    """Latent shape, raw uint16 layer lengths and the layer payloads -> one l3ic stream (bytes)."""
    n = len(payloads)
    head = struct.pack('<3BH{}H'.format(n), h, w, n, 2 * n, *[len(p) for p in payloads])
    return head + b''.join(bytes(p) for p in payloads)


def parse_container(stream):
    """bytes -> (h, w, n, [payload bytes]); raises L3ICError on a malformed container."""
    stream = bytes(stream)
    if len(stream) < 5:
        raise L3ICError('Truncated stream ({} bytes)'.format(len(stream)))
    h, w, n = stream[0], stream[1], stream[2]
    (nl,) = struct.unpack_from('<H', stream, 3)
    if nl != 2 * n:
        raise L3ICError('Entropy-coded layer lengths are not supported ({} bytes for {} layers)'.format(nl, n))
    if len(stream) < 5 + 2 * n:
        raise L3ICError('Truncated stream ({} bytes)'.format(len(stream)))
    lengths = struct.unpack_from('<{}H'.format(n), stream, 5)
    pos, payloads = 5 + 2 * n, []
    for ln in lengths:
        payloads.append(stream[pos:pos + ln])
        pos += ln
    if pos != len(stream):
        raise L3ICError('Stream of {} bytes, its layers account for {}'.format(len(stream), pos))
    return h, w, n, payloads


# ---- latent <-> bytes -----------------------------------------------------------------------------------------------
def _device_codebook(codebook, device):
    cb = codebook.t if isinstance(codebook, DeviceArray) else codebook
    if isinstance(cb, torch.Tensor):
        return cb.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(cb, dtype=np.float32).reshape(-1))).to(device)


def _model_codebook(model, device):
    cb = getattr(model, '_codebook', None)
    return _device_codebook(cb if cb is not None else model.get_codebook(), device)


def _encode(z, codebook, want_stats=False):
    z = z.t if isinstance(z, DeviceArray) else z
    shape = tuple(z.shape)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4:
        raise ValueError('A (B, H, W, N) latent expected, got shape {}'.format(tuple(z.shape)))
    b, h, w, n = shape
    k = (codebook.t if isinstance(codebook, DeviceArray) else codebook).reshape(-1).shape[0]
    check_latent_shape(h, w, n, k)                               # before any device work
    dev = z.device if isinstance(z, torch.Tensor) and z.is_cuda else default_device()
    z = to_device(z, dev).reshape(shape).float().contiguous()
    cb = _device_codebook(codebook, dev)
    idx, bad = ops.l3ic_quantise(z, cb)
    data, lengths, hist, _ = ops.l3ic_encode(idx, want_stats=want_stats)
    small = torch.cat([bad, lengths]).cpu().numpy()            # the one synchronisation
    if small[0]:
        raise L3ICError('The latent holds non-finite values')
    lengths = small[1:].astype(np.int64)
    blob = data[:int(lengths.sum())].cpu().numpy().tobytes()
    ends = np.cumsum(lengths)
    streams = []
    for i in range(b):
        lo = int(ends[i * n - 1]) if i else 0
        cuts = [lo] + [int(e) for e in ends[i * n:(i + 1) * n]]
        streams.append(pack_container(h, w, [blob[cuts[j]:cuts[j + 1]] for j in range(n)]))
    return streams, (hist.view(b, n, 256) if hist is not None else None)


def encode_latent(z, codebook):
    """A latent batch (B, H, W, N) -> one l3ic stream (bytes) per image: quantised to the codebook and entropy coded on
    the GPU in one set of launches."""
    return _encode(z, codebook)[0]


def decode_latent(streams, codebook, device=None):
    """l3ic streams (all of one latent shape) -> the (B, H, W, N) float32 device latent codebook[index], decoded on the GPU
    in one launch."""
    if isinstance(streams, (bytes, bytearray, memoryview)):
        streams = [streams]
    dev = device or default_device()
    cb = _device_codebook(codebook, dev)
    parsed = [parse_container(s) for s in streams]
    if not parsed:
        raise L3ICError('No streams to decode')
    h, w, n = parsed[0][:3]
    for i, p in enumerate(parsed):
        if p[:3] != (h, w, n):
            raise L3ICError('Image {}: latent {}x{}x{}, expected {}x{}x{} like image 0'.format(i, *p[:3], h, w, n))
    check_latent_shape(h, w, n, cb.numel())
    payloads = [pl for p in parsed for pl in p[3]]
    lengths = np.array([len(pl) for pl in payloads], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    blob = np.frombuffer(b''.join(payloads) or b'\0', np.uint8)
    meta = torch.from_numpy(np.concatenate([offsets, lengths]).astype(np.int32)).to(dev)
    data = torch.from_numpy(blob.copy()).to(dev)
    z, err = ops.l3ic_decode(data, meta[:len(payloads)], meta[len(payloads):], cb, (len(parsed), h, w, n))
    err = err.cpu().numpy()                                      # the one synchronisation
    if err.any():
        s = int(np.flatnonzero(err)[0])
        why = ', '.join(v for k, v in sorted(ops.L3IC_ERRORS.items()) if err[s] & k)
        raise L3ICError('Image {} layer {}: malformed layer payload ({}){}'.format(
            s // n, s % n, why, '' if np.count_nonzero(err) == 1 else ' - {} layers in all'.format(np.count_nonzero(err))))
    return z


def compress_batch(batch_x, model):
    """A batch of images -> one l3ic stream per image: model.compress, then encode_latent."""
    z = model.compress(batch_x)
    return encode_latent(z, _model_codebook(model, z.t.device))


def decompress_batch(streams, model):
    """l3ic streams -> the decoded images (B, H, W, 3) as a numpy array: decode_latent, then model.decompress."""
    z = decode_latent(streams, _model_codebook(model, model.device), device=model.device)
    return model.decompress(z).numpy()


# ---- the reference's surface ----------------------------------------------------------------------------------------
def simulate_compression(batch_x, dcn):
    """Compress and decompress one image (through bytes).  Returns the decompressed image and the byte count."""
    compressed_image = compress(batch_x, dcn)
    batch_y = decompress(compressed_image, dcn)
    return batch_y, len(compressed_image)


def compress_n_stats(batch_x, dcn):
    """Per-image SSIM, PSNR, latent entropy, coded bytes and bits per pixel of a batch coded through l3ic streams (scalars
    for a batch of one).  'entropy' is helpers/stats.py:119-131 of the reference - the codebook histogram of the image's
    whole latent, counts clipped at 1, in bits - taken from the encoder's device histograms.  It equals the reference's
    np.histogram count on hard-quantised latents; it differs only for values exactly at a codebook midpoint (here the
    lower entry, there the upper bin) and beyond twice the codebook range (dropped there, clamped to the end entry here)."""
    batch_x = np.asarray(batch_x, dtype=np.float32)
    if batch_x.ndim == 3:
        batch_x = batch_x[None]
    z = dcn.compress(batch_x)
    streams, hist = _encode(z, _model_codebook(dcn, z.t.device), want_stats=True)
    batch_y = decompress_batch(streams, dcn)
    k = len(dcn.get_codebook())
    counts = hist.sum(dim=1).cpu().numpy()[:, :k].astype(np.float64).clip(min=1)
    probs = counts / counts.sum(axis=1, keepdims=True)
    n_bytes = np.array([len(s) for s in streams], np.float64)
    h, w = batch_x.shape[1], batch_x.shape[2]
    stats = {
        'ssim': np.atleast_1d(metrics.ssim(batch_x, batch_y)).astype(np.float64),
        'psnr': np.atleast_1d(metrics.psnr(batch_x, batch_y)).astype(np.float64),
        'entropy': -np.sum(probs * np.log2(probs), axis=1),
        'bytes': n_bytes,
        'bpp': 8 * n_bytes / h / w,
    }
    if batch_x.shape[0] == 1:
        for key in stats.keys():
            stats[key] = stats[key][0]
    return batch_y, stats


def compress(batch_x, model, verbose=False):
    """Serialise one image as an l3ic stream (bytes); the feature layers are coded separately (module docstring)."""
    if batch_x.ndim == 3:
        batch_x = np.expand_dims(batch_x, axis=0)
    assert batch_x.ndim == 4
    assert batch_x.shape[0] == 1
    stream = compress_batch(batch_x, model)[0]
    if verbose:
        h, w, n, payloads = parse_container(stream)
        print('[l3ic encoder]', 'Latent space', h, w, n)
        print('[l3ic encoder]', 'Layer lengths = ', [len(p) for p in payloads])
    return stream


def decompress(stream, model=None, verbose=False):
    """Decompress an image from an l3ic stream (bytes or a file-like object).  Returns (1, H, W, 3) numpy."""
    if isinstance(stream, (bytes, bytearray, memoryview)):
        stream = bytes(stream)
    elif hasattr(stream, 'read'):
        stream = stream.read()
    else:
        raise ValueError('Unsupported stream type!')
    h, w, n_latent, payloads = parse_container(stream)
    if verbose:
        print('[l3ic decoder]', 'Latent space', h, w, n_latent)
        print('[l3ic decoder]', 'Layer lengths', [len(p) for p in payloads])
    if model is None:
        model = restore('{}c'.format(n_latent))
    if model.latent_shape[-1] != n_latent:
        print('[l3ic decoder]', 'WARNING', 'the specified model ({}c) does not match the coded stream ({}c) - switching'.format(
            model.latent_shape[-1], n_latent))
        model = restore('{}c'.format(n_latent))
    return decompress_batch([stream], model)


def restore(dir_name, patch_size=None, fetch_stats=False):
    """Restore a trained DCN from its training directory (the reference's wrapper over tfmodel.restore, key 'codec')."""
    from ..models import compression
    if dir_name is None or not Path(dir_name).exists():
        raise ValueError('Directory {} does not exist!'.format(dir_name))
    logs = sorted(Path(dir_name).glob('**/*.json'))
    name = 'TwitterDCN'
    if logs:
        with open(str(logs[0])) as f:
            name = json.load(f).get('codec', {}).get('model', name)
    model = getattr(compression, name).restore(dir_name, key='codec', patch_size=patch_size)
    if not fetch_stats:
        return model
    stats = {}
    for k, v in getattr(model, 'performance', {}).items():
        if 'validation' in v and len(v['validation']) > 0:
            stats[k] = np.round(v['validation'][-1], 3)
        elif 'training' in v and len(v['training']) > 0:
            stats[k] = np.round(v['training'][-1], 3)
    return model, stats
