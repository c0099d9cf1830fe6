"""
JPEG helpers with the reference's names (compression/jpeg_helpers.py).

  jpeg_qtable, zigzag, jpeg_qf_estimation (:253-310)   the tables of the differentiable codec; jpeg_qtable goes through the native
                                                        library (nimg_jpeg_qtable), tested bit-exactly against the reference
  compress_batch (:82-114), match_quality (:26-79)      the standard codec - the reference's imageio / libjpeg round trip - on the
                                                        GPU kernels nimg_jpeg_* (format: DESIGN.md section 4c, libjpeg's byte for byte)
  encode_batch                                          new: the files themselves
  optimize=True (compress_batch, encode_batch,          new: files with optimised Huffman tables, libjpeg's optimize_coding byte for
  rate_distortion, match_quality[_batch])               byte - histograms, tables and coding per image on the GPU
  parse_header, decode_batch, decode_coefficients       new: the way back - any baseline file (its own quantisation and Huffman tables,
                                                        optimised ones included) decoded on the GPU to the bytes imageio.imread returns;
                                                        headers are parsed on the host, the entropy decoder is the parallel Huffman
                                                        decoder of DESIGN.md section 4e (nimg_jpeg_decode, nimg_jpeg_reconstruct_tables)
  rate_distortion, match_quality_batch                  new: a whole quality sweep / the bisection of every image of a batch through
                                                        the item kernels (one quality per item)
  qtables= (jpeg_header, device_codec, encode_batch,    new: files with any 8-bit quantisation tables in place of a quality - learned
  compress_batch), check_qtables,                       ones, the differentiable codec's, a foreign file's;
  rate_distortion_tables, transcode_batch               K table sets over a batch in one item call; a file written again with its
                                                        coefficients and tables untouched and optimal (or Annex K) Huffman tables
  restart_interval= (jpeg_header, device_codec,         new: files with restart intervals, libjpeg's byte for byte, and - asked for with
  encode_batch, compress_batch), allow_restart=         allow_restart - read back with every interval as an entry point of the parallel
  (parse_header, decode_batch, decode_coefficients,     decoder
  transcode_batch)
  progressive= (jpeg_header, device_codec,              new: progressive files (SOF2), the ten scans of libjpeg's simple progression
  encode_batch, compress_batch, transcode_batch),       byte for byte, every scan with a Huffman table of its own;
  jpeg_progressive_pieces                               written only - parse_header refuses them as before
  (n,h,w,1) input (jpeg_header 'grey', device_codec,    new: grey-scale files - one component, what libjpeg writes for a mode 'L' image byte
  encode_batch, compress_batch), allow_grey=            for byte - written as baseline files and, asked for with allow_grey, read back,
  (parse_header, decode_batch, decode_coefficients,     baseline or progressive, next to colour files in one call
  transcode_batch)
  lossless=, edge=, crop= (transcode_batch),           new: jpegtran's lossless transforms - flips, transposition, rotations, the aligned crop -
  lossless_size                                         on the coefficients, one memory pass on the device
  JPEGMarkerStats (:133-250)                            host parsing of a file's segments

JPEG 2000 sizes (jp2bytes :117-125) stay out of scope.
"""
import functools
import re
import struct
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from .. import ops
from ..device import default_device, unwrap

JPEG_HEADER_BYTES = 623           # SOI .. SOS of every file written here with two quantisation tables
_DRI_BYTES = 6                    # a restart interval (restart_interval= above 0): one DRI segment between the last DHT and SOS
_DHT_OFFSET = 177
_DQT_BYTES = 69                   # a third quantisation table (qtables= with three): one more DQT segment in front of SOF0

# The four Annex K Huffman table segments as libjpeg writes them (ids 00, 10, 01, 11): 16 counts, then the symbols.
_DHT = tuple(bytes.fromhex(t) for t in (
    '00' '00010501010101010100000000000000' '000102030405060708090a0b',
    '10' '0002010303020403050504040000017d'
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738'
    '393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5'
    'a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa',
    '01' '00030101010101010101010000000000' '000102030405060708090a0b',
    '11' '00020102040403040705040400010277'
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637'
    '38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3'
    'a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))

_BASE_TABLES = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56) + (99,) * 5 + (47, 66) + (99,) * 38)


def jpeg_qtable(quality, channel=0):
    """DCT quantisation matrix for a quality level 1..100; channel 0 = luma, >0 = chroma. Returns (8,8) float32."""
    return ops.qtable(int(np.maximum(np.minimum(100, quality), 1)), int(channel))


def zigzag(n):
    """Zig-zag scan index matrix (jpeg_helpers.py:253-261): entry [r, c] = position of coefficient (r, c) in the scan.  The
    scan walks the anti-diagonals d = r + c in order; odd diagonals run top-right -> bottom-left (r ascending), even ones the
    other way."""
    r, c = np.divmod(np.arange(n * n), n)
    d = r + c
    order = np.lexsort((np.where(d % 2 == 1, r, -r), d))          # primary key d, secondary the walking direction
    zz = np.empty(n * n, dtype=np.uint16)
    zz[order] = np.arange(n * n, dtype=np.uint16)
    return zz.reshape(n, n)


def jpeg_qf_estimation(q_mtx, channel=0):
    """The IJG quality 1..100 whose table of `channel` is closest (mean absolute difference) to q_mtx; ties -> the lowest."""
    tables = np.stack([jpeg_qtable(qf, channel) for qf in range(1, 101)]).astype(np.float64)
    return 1 + int(np.abs(tables - np.asarray(q_mtx, dtype=np.float64)).mean(axis=(1, 2)).argmin())


# ---- the standard codec ---------------------------------------------------------------------------------------------------
def libjpeg_qtable(quality, channel=0):
    """The table libjpeg itself writes for a quality 1..100, (8,8) int64.  jpeg_qtable above scales by the real number 5000 / q as
    the reference's Python does; libjpeg divides in integers, so entries differ by 1 or 2 at many qualities below 50 that do
    not divide 5000.  The files and the kernels (csrc/jpegc.hip make_qtabs) use libjpeg's."""
    quality = int(min(100, max(1, quality)))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    t = (np.array(_BASE_TABLES[0 if channel == 0 else 1], np.int64) * scale + 50) // 100
    return np.clip(t, 1, 255).reshape(8, 8)


def check_qtables(qtables, grey=False):
    """Quantisation tables as a baseline file carries them: two (luma, chroma) or three (Y, Cb, Cr) tables of 64 integers 1..255 in
    natural (row-major) order, given as (T, 64) or (T, 8, 8) -> (T, 64) uint16.  Everything else is a ValueError that names the
    table and the entry.  (Larger entries would need 16-bit DQT segments and an SOF1 frame: not written here.)  `grey`: the tables of
    a grey-scale file - one, or two or three of which the first alone is used and written, as libjpeg does -> (1, 64)."""
    try:
        t = np.asarray(qtables)
        numeric = np.issubdtype(t.dtype, np.number) or t.dtype == np.bool_
    except Exception:
        numeric = False
    if not numeric:
        raise ValueError('qtables: two or three tables of 64 numbers needed, got {}'.format(type(qtables).__name__))
    if t.ndim == 3 and t.shape[1:] == (8, 8):
        t = t.reshape(t.shape[0], 64)
    if t.ndim != 2 or t.shape[1] != 64:
        raise ValueError('qtables: shape (T, 64) or (T, 8, 8) needed, got {}'.format(tuple(np.shape(qtables))))
    if grey:
        if t.shape[0] not in (1, 2, 3):
            raise ValueError('qtables: 1 table needed for a grey-scale file (of 2 or 3 the first is used), got {}'.format(t.shape[0]))
        t = t[:1]
    elif t.shape[0] not in (2, 3):
        raise ValueError('qtables: 2 tables (luma, chroma) or 3 (Y, Cb, Cr) needed, got {}'.format(t.shape[0]))
    t = t.astype(np.float64)
    with np.errstate(invalid='ignore'):
        bad = ~np.isfinite(t) | (t != np.rint(t)) | (t < 1) | (t > 255)
    if bad.any():
        k, e = (int(v[0]) for v in np.nonzero(bad))
        raise ValueError('qtables: entry {} (row {}, column {}) of table {} is {}: integers 1..255 needed (a baseline file has 8-bit '
                         'tables)'.format(e, e // 8, e % 8, k, t[k, e]))
    return t.astype(np.uint16)


def _quality_or_tables(quality, qtables, clamp=False, grey=False):
    """Exactly one of the two says what a file is quantised with -> (quality 1..100 or None, (T, 64) uint16 or None); checked on the
    host, before anything is uploaded.  A quality outside 1..100 is refused, or with `clamp` left to libjpeg_qtable's clamp.
    `grey`: the tables are those of a grey-scale file (check_qtables)."""
    if (quality is None) == (qtables is None):
        raise ValueError('either a quality or qtables= is needed, {} were given'.format('both' if qtables is not None else 'neither'))
    if qtables is not None:
        return None, check_qtables(qtables, grey)
    if clamp:
        return quality, None
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('Invalid JPEG quality: {}'.format(q))
    return q, None


JPEG_GREY_HEADER_BYTES = 328      # SOI .. SOS of a grey-scale file: one DQT, an SOF0 and an SOS of one component, the two luma DHT
_GREY_DHT_OFFSET = 102


def _header_bytes(tables, restart_interval=0, grey=False):
    """(bytes from SOI to the end of SOS with the Annex K Huffman tables, offset of the first DHT segment) of a file with
    `tables` = None or (2, 64): 623 and 177; (3, 64): one DQT segment more.  A restart interval adds its DRI segment's 6 bytes behind
    the Huffman tables.  `grey`: 328 and 102, whatever the tables."""
    if grey:
        return JPEG_GREY_HEADER_BYTES + (_DRI_BYTES if restart_interval else 0), _GREY_DHT_OFFSET
    extra = _DQT_BYTES if tables is not None and len(tables) == 3 else 0
    return JPEG_HEADER_BYTES + extra + (_DRI_BYTES if restart_interval else 0), _DHT_OFFSET + extra


def jpeg_header(h, w, quality, subsampling='4:4:4', huffman=None, qtables=None, *, restart_interval=0, progressive=False):
    """The bytes from SOI to the end of SOS as libjpeg writes them: 623 with default settings.  huffman: one image's four tables in
    DHT-id order 00 10 01 11 as (4, 272) bytes (16 counts, then the symbols in code order) - what libjpeg writes with optimize_coding:
    four DHT segments of 21 bytes + the table's symbols each.  The first DHT segment stays at offset 177.  qtables (with quality None,
    see check_qtables): these tables instead of a quality's, as libjpeg writes a caller's - zig-zag, one DQT segment each; a third
    table goes to Cr (selector 2 in SOF0) and moves everything behind it by 69 bytes: 692 in all, the first DHT at 246.
    restart_interval (MCUs, 0..65535): above 0 the DRI segment FFDD 0004 RRRR between the last DHT segment and SOS, 6 bytes more.
    subsampling 'grey': the header of a grey-scale file - one DQT segment (table 0: the quality's luma table, or
    the first of qtables), SOF0 and SOS of one component (id 1, sampling 1x1), the DC and AC table 0 - Annex K's, or huffman (2, 272).
    progressive: the bytes in front of the FIRST scan of a progressive file - SOF2 in place of SOF0, the two DC tables of huffman
    (10, 272) (which is needed: a progressive file has no default tables), the DRI segment, the first SOS; jpeg_progressive_pieces
    gives what stands in front of every scan."""
    if progressive:
        return jpeg_progressive_pieces(h, w, quality, subsampling, huffman, qtables=qtables, restart_interval=restart_interval)[0]
    return _jpeg_header(h, w, quality, subsampling, huffman, qtables, restart_interval)


# libjpeg's jpeg_simple_progression for three components: (component 0 Y, 1 Cb, 2 Cr or None = all interleaved, Ss, Se, Ah, Al, which of
# the image's ten tables is written in front of the scan).  Cr comes before Cb.
_PROGRESSIVE_SCANS = ((None, 0, 0, 0, 1, None), (0, 1, 5, 0, 2, 2), (2, 1, 63, 0, 1, 3), (1, 1, 63, 0, 1, 4), (0, 6, 63, 0, 2, 5),
                      (0, 1, 63, 2, 1, 6), (None, 0, 0, 1, 0, None), (2, 1, 63, 1, 0, 7), (1, 1, 63, 1, 0, 8), (0, 1, 63, 1, 0, 9))


def _dht_segment(ident, table):
    body = bytes([ident]) + table[:16 + int(table[:16].sum(dtype=np.int64))].tobytes()
    return b'\xff\xc4' + struct.pack('>H', len(body) + 2) + body


_ANNEX_K_DHT = b''.join(_dht_segment(t[0], np.frombuffer(t, np.uint8, offset=1)) for t in _DHT)
_GREY_DHT_BYTES = 33 + 183        # the first two of them, the luma tables: all a grey-scale file carries
_ANNEX_K_SYMBOLS, _GREY_ANNEX_K_SYMBOLS = 348, 174       # the symbols of the four tables, and of the two


def _colour_only(what, grey):
    """What DESIGN.md section 8 lists as out for grey-scale (one-component) input says so."""
    if grey:
        raise ValueError('grey-scale (one-component) images: {} is not supported'.format(what))


_PROGRESSIVE_GREY = 'progressive=True (writing the six scans libjpeg writes for one component)'


def _factors(subsampling):
    """The factors (hs, vs) of what a caller names a geometry by: a name of ops.JPEG_SUBSAMPLING or 'grey' (ops.jpeg_subsampling: by name the
    samplings that are only read stay refused, as writing them from pixels is), or the factors themselves - ops.JPEG_GREY and the pairs
    of ops.JPEG_SAMPLING_WIDE too, which transcode_batch passes for the file it writes again."""
    return subsampling if isinstance(subsampling, tuple) else ops.jpeg_subsampling(subsampling)


def _grey_shape(shape):                  # an image (h,w,1) or a batch (n,h,w,1): one component
    return len(shape) in (3, 4) and shape[-1] == 1


def _grey_input(shape, subsampling, name):
    """The sub-sampling a batch of `shape` is coded with: 'grey' for (..., 1) - which takes no other than the default or 'grey' itself,
    there being no chroma to sub-sample -, else `subsampling`, which is then not 'grey'."""
    if _grey_shape(shape):
        if subsampling not in ('4:4:4', 'grey'):
            raise ValueError('{}: grey-scale input {} takes no chroma sub-sampling, got {!r}'.format(name, tuple(shape), subsampling))
        return 'grey'
    if subsampling == 'grey':
        raise ValueError("{}: subsampling 'grey' needs (n,h,w,1) or (h,w,1) input, got {}".format(name, tuple(shape)))
    return subsampling


def _dri_segment(ri):
    """FFDD 0004 RRRR; nothing for interval 0."""
    return b'\xff\xdd\x00\x04' + struct.pack('>H', ri) if ri else b''


def jpeg_progressive_pieces(h, w, quality, subsampling='4:4:4', huffman=None, qtables=None, *, restart_interval=0):
    """What stands in front of each of the ten entropy-coded segments of a progressive file, a list of ten bytes objects: [0] SOI,
    APP0, the DQT segments, SOF2, the DC tables 00 and 01, the DRI segment, the first SOS; [k] the DHT segment of scan k's AC table
    (none in front of the DC refine scan) and its SOS.  huffman: the image's ten tables (10, 272) in the order of these DHT segments.
    file = pieces[0] + segment 0 + ... + pieces[9] + segment 9 + FFD9."""
    huffman = None if huffman is None else np.asarray(huffman)
    if huffman is None or huffman.dtype != np.uint8 or huffman.shape != (ops.JPEG_PROGRESSIVE_SCANS, 272):
        raise ValueError('huffman: the (10, 272) uint8 tables of a progressive file are needed, got {}'.format(
            None if huffman is None else (huffman.dtype, huffman.shape)))
    ri = ops.jpeg_restart_interval(restart_interval)
    _colour_only(_PROGRESSIVE_GREY, ops.jpeg_is_grey(*_factors(subsampling)))
    base = _jpeg_header(h, w, quality, subsampling, None, qtables, 0)
    dht = _header_bytes(None if qtables is None else check_qtables(qtables))[1]
    sof = dht - 19
    assert base[sof:sof + 2] == b'\xff\xc0'
    first = base[:sof] + b'\xff\xc2' + base[sof + 2:dht] + _dht_segment(0x00, huffman[0]) + _dht_segment(0x01, huffman[1]) + _dri_segment(ri)
    pieces = []
    for comp, ss, se, ah, al, table in _PROGRESSIVE_SCANS:
        if comp is None:
            dc = 0x10 if ah == 0 else 0x00
            piece = bytes([0xff, 0xda, 0, 12, 3, 1, 0, 2, dc, 3, dc])
        else:
            piece = _dht_segment(0x10 | (comp != 0), huffman[table]) + bytes([0xff, 0xda, 0, 8, 1, comp + 1, int(comp != 0)])
        pieces.append(piece + bytes([ss, se, (ah << 4) | al]))
    pieces[0] = first + pieces[0]
    return pieces


def _jpeg_header(h, w, quality, subsampling, huffman, qtables, restart_interval):
    hs, vs = _factors(subsampling)
    grey = ops.jpeg_is_grey(hs, vs)
    ri = ops.jpeg_restart_interval(restart_interval)
    quality, qtables = _quality_or_tables(quality, qtables, clamp=True, grey=grey)
    if qtables is None:
        qtables = np.stack([libjpeg_qtable(quality, t).ravel() for t in ((0,) if grey else (0, 1))])
    order = np.argsort(zigzag(8).ravel(), kind='stable')                 # scan position -> natural index
    out = bytes.fromhex('ffd8' 'ffe00010' '4a46494600' '0101' '00' '0001' '0001' '0000')
    for t, table in enumerate(qtables):
        out += bytes.fromhex('ffdb0043') + bytes([t]) + table[order].astype(np.uint8).tobytes()
    idents = (0x00, 0x10) if grey else (0x00, 0x10, 0x01, 0x11)          # the luma tables are all a grey-scale file carries
    dht = _ANNEX_K_DHT[:_GREY_DHT_BYTES] if grey else _ANNEX_K_DHT
    if huffman is not None:
        huffman = np.asarray(huffman)
        if huffman.dtype != np.uint8 or huffman.shape != (len(idents), 272):
            raise ValueError('huffman: ({}, 272) uint8 needed{}, got {} {}'.format(len(idents), ' for a grey-scale file' if grey else '',
                                                                                   huffman.dtype, huffman.shape))
        dht = b''.join(_dht_segment(ident, t) for ident, t in zip(idents, huffman))
    if grey:
        return out + bytes.fromhex('ffc0000b' '08') + struct.pack('>HH', h, w) + bytes([1, 1, 0x11, 0]) + dht + _dri_segment(ri) + \
            bytes.fromhex('ffda0008' '01' '0100' '00' '3f' '00')
    out += bytes.fromhex('ffc00011' '08') + struct.pack('>HH', h, w) + bytes([3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, len(qtables) - 1])
    return out + dht + _dri_segment(ri) + bytes.fromhex('ffda000c' '03' '0100' '0211' '0311' '00' '3f' '00')


def _device_batch(batch_x, keep_bytes, device=None):
    """numpy / DeviceArray / torch (n,h,w,3) -> contiguous device tensor: uint8 as it is when keep_bytes, everything else float32
    (the kernel then applies the reference's conversion, jpeg_helpers.py:92-97)."""
    x = unwrap(batch_x)
    if not isinstance(x, torch.Tensor):
        x = np.ascontiguousarray(x if (keep_bytes and x.dtype == np.uint8) else np.asarray(x, dtype=np.float32))
        x = torch.from_numpy(x if x.flags.writeable else x.copy())          # (torch refuses to wrap read-only memory quietly)
    dtype = torch.uint8 if (keep_bytes and x.dtype == torch.uint8) else torch.float32
    dev = x.device if x.is_cuda else (device if device is not None else default_device())
    return x.to(device=dev, dtype=dtype).contiguous()


JPEG_OPT_STATUS_BITS = OrderedDict([(1, 'Huffman table that is no prefix code'), (2, 'symbol without a code'),
                                    (4, 'Huffman code size above 32'), (8, 'symbol histogram total of 2^32 or more')])


def _coding(optimize=False, progressive=False):
    """What codes a batch in a mode: (the op that counts the symbols of its tables, None = the Annex K tables; the encode op; the bound
    of one image's segments).  Looked up in ops when asked, so that what is set there holds."""
    if progressive:
        return ops.jpeg_progressive_histogram, ops.jpeg_encode_progressive, ops.jpeg_progressive_ecd_bound
    if optimize:
        return ops.jpeg_histogram, ops.jpeg_encode_tables, ops.jpeg_ecd_bound_tables
    return None, ops.jpeg_encode, ops.jpeg_ecd_bound


def _optimised(coding, coef, h, w, hs, vs, capacity, restart_interval=0):
    """histogram -> optimal tables -> encode on the device with the ops of `coding` (_coding: 4 tables per image, or the 10 of a
    progressive file): (segments, lengths (n,) or (n, 10) int32, tables (n, T, 272) uint8, status (n,) int32: the bits of
    JPEG_OPT_STATUS_BITS).  Nothing is read back."""
    histogram, encode, _ = coding
    tables, tstatus = ops.jpeg_optimal_tables(histogram(coef, h, w, hs, vs, restart_interval=restart_interval))
    data, lengths, status = encode(coef, tables, h, w, hs, vs, capacity=capacity, restart_interval=restart_interval)
    return data, lengths, tables, status | (functools.reduce(torch.bitwise_or, tstatus.unbind(1)) << 2)


def _raise_on_opt_status(status):
    bad = [(i, int(s)) for i, s in enumerate(np.asarray(status).tolist()) if s]
    if bad:
        raise ValueError('optimised Huffman coding failed for image(s) {}: {}'.format(
            [i for i, _ in bad], '; '.join('{}: status {} ({})'.format(
                i, s, ' | '.join(text for bit, text in JPEG_OPT_STATUS_BITS.items() if s & bit)) for i, s in bad)))


def _device_segments(coding, coef, n, h, w, hs, vs, ws=None, restart_interval=0):
    """The entropy-coded segments of a batch in the mode of `coding` (_coding) -> (segments, tables): per image its segment as bytes, or
    a list of the ten of a progressive file; the tables (n, T, 272) uint8 numpy, None for Annex K's.  One download for the lengths -
    status and tables, where the mode has them, come in the same copy -, one for the segments.  `ws`: a workspace of
    ops.jpeg_workspace_bytes the encoder may use (without tables: theirs is another)."""
    histogram, encode, bound = coding
    # room for 3 bytes per sample (random noise at quality 100 needs about 2); the bound is 6.5, and a batch that needs more
    # than it was given reports so through its lengths and is coded again with exactly what it needs
    capacity = n * min(bound(h, w, hs, vs, restart_interval), 192 * ops.jpeg_geometry(h, w, hs, vs)[1] + 1024)
    if histogram is None:
        tables, again = None, functools.partial(encode, coef, h, w, hs, vs, workspace=ws, restart_interval=restart_interval)
        data, lengths = again(capacity=capacity)
        shape, lengths = tuple(lengths.shape), lengths.cpu().numpy().astype(np.int64)
    else:
        data, lengths, tables, status = _optimised(coding, coef, h, w, hs, vs, capacity, restart_interval)
        again = functools.partial(encode, coef, tables, h, w, hs, vs, restart_interval=restart_interval)
        shape, words = tuple(lengths.shape), lengths.numel()
        flat = torch.cat([lengths.reshape(-1).view(torch.uint8), status.view(torch.uint8), tables.reshape(-1)]).cpu().numpy()
        lengths, status = flat[:4 * words].view(np.int32).astype(np.int64), flat[4 * words:4 * (words + n)].view(np.int32)
        _raise_on_opt_status(status)
        tables = flat[4 * (words + n):].reshape(tuple(tables.shape))
    total = int(lengths.sum())
    if total > capacity:
        data = again(capacity=total)[0]
    blob = data[:total].cpu().numpy().tobytes()
    ends = np.concatenate([[0], np.cumsum(lengths)])
    pieces = [blob[a:b] for a, b in zip(ends[:-1], ends[1:])]
    return (pieces if len(shape) == 1 else [pieces[i * shape[1]:(i + 1) * shape[1]] for i in range(n)]), tables


def _device_tables(tables, items, device):
    """Table sets (K, T, 64) uint16 of check_qtables -> the (K * items, 3, 64) device tensor the table kernels read, set-major: every
    set repeated for `items` consecutive items; with two tables Cr takes the chroma table.  The one table of a grey-scale file stays
    one: (K * items, 1, 64)."""
    t = np.asarray(tables)
    t = t[:, [0, 1, 1]] if t.shape[1] == 2 else t
    return torch.from_numpy(np.repeat(t, items, axis=0).view(np.int16)).to(device)


def device_codec(x, quality, subsampling='4:4:4', want_image=True, want_bytes=True, optimize=False, *, qtables=None, restart_interval=0,
                 progressive=False):
    """One batch through the GPU codec: x (n,h,w,3) device tensor, float32 or uint8 -> (decoded (n,h,w,3) float32 device tensor or
    None, list of the entropy-coded segments as bytes or None).  One host synchronisation (for the lengths) when want_bytes.
    With `optimize` the segments are coded with per-image optimal Huffman tables (histogram -> optimal tables -> encode_tables, the
    tables and the lengths coming back together) and a third value is returned: the tables, (n, 4, 272) uint8, or None.
    qtables (with quality None, see check_qtables): the whole batch is quantised with these tables instead of a quality's
    (ops.jpeg_transform_tables, ops.jpeg_reconstruct_tables).  restart_interval (MCUs, 0..65535): the segments carry a restart marker
    behind every so many MCUs; the image is the same.  progressive: the ten scans of a progressive file
     - `segments` is then a list of ten bytes objects per image and the tables, (n, 10, 272), are always
    returned as the third value: a progressive file has optimised tables with `optimize` or without.
    x (n,h,w,1): a grey-scale batch - subsampling left at its default or 'grey', the image (n,h,w,1), the tables
    (n, 2, 272), qtables one table (or the first of two or three); not with `progressive`."""
    subsampling = _grey_input(x.shape, subsampling, 'device_codec')
    hs, vs = ops.jpeg_subsampling(subsampling)
    grey = ops.jpeg_is_grey(hs, vs)
    _colour_only(_PROGRESSIVE_GREY, grey and progressive)
    quality, qtables = _quality_or_tables(quality, qtables, grey=grey)
    ri = ops.jpeg_restart_interval(restart_interval)
    n, h, w, _ = x.shape
    ws = torch.empty(ops.jpeg_workspace_bytes(n, h, w, hs, vs, ri) or 1, dtype=torch.uint8, device=x.device)
    if qtables is None:
        coef = ops.jpeg_transform(x, quality, hs, vs, workspace=ws)
    else:
        qt = _device_tables(qtables[None], n, x.device)
        coef = ops.jpeg_transform_tables(x, qt, hs, vs, workspace=ws)[0]          # (check_qtables has seen every entry: no flag to read)
    segments = tables = None
    if want_bytes:
        segments, tables = _device_segments(_coding(optimize, progressive), coef, n, h, w, hs, vs, ws, ri)
    image = None
    if want_image and grey and qtables is None:          # the one reconstruction of a grey-scale batch takes the table itself
        qt = _device_tables(libjpeg_qtable(quality, 0).reshape(1, 1, 64).astype(np.uint16), n, x.device)
        image = ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs, workspace=ws)
    elif want_image:
        image = ops.jpeg_reconstruct(coef, h, w, quality, hs, vs, workspace=ws) if qtables is None else \
            ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs, workspace=ws)
    return (image, segments, tables) if optimize or progressive else (image, segments)


def encode_batch(batch_x, quality, subsampling='4:4:4', optimize=False, *, qtables=None, restart_interval=0, progressive=False):
    """The JPEG files of a batch (n,h,w,3) or one image (h,w,3), a list of bytes.  uint8 input is coded as it is; float input goes
    through the reference's conversion (x / 255 first if its maximum exceeds 1, then (255 x) truncated).  `optimize`: every file with
    Huffman tables of its own, the files libjpeg writes with optimize_coding (Pillow: optimize=True).  qtables (with quality None, see
    check_qtables): the files libjpeg writes with these quantisation tables (Pillow: qtables=[...]).  restart_interval (MCUs in
    scan order, 0..65535): the files libjpeg writes with that restart interval (Pillow: restart_marker_blocks=) - a DRI segment and a
    marker FFD0..FFD7 behind every so many MCUs that another follows; a whole number of MCU rows is rows * MCUs per row.
    progressive: the files libjpeg writes with jpeg_simple_progression (Pillow: progressive=True) - SOF2 and ten scans, each with an
    optimal table of its own, the same bytes with `optimize` or without; in a single-component scan the restart interval counts
    blocks.  (n,h,w,1) or (h,w,1): grey-scale files, the ones libjpeg writes for a mode 'L' image - subsampling
    left at its default or 'grey', qtables one table (or the first of two or three), not with `progressive`."""
    shape = np.shape(unwrap(batch_x))
    subsampling = _grey_input(shape, subsampling, 'encode_batch')                               # (host checks first: nothing is uploaded
    quality, qtables = _quality_or_tables(quality, qtables, grey=_grey_shape(shape))            # for a call that is refused)
    ri = ops.jpeg_restart_interval(restart_interval)
    x = _device_batch(batch_x, keep_bytes=True)
    if x.dim() == 3:
        x = x[None]
    _, segments, tables = (device_codec(x, quality, subsampling, want_image=False, optimize=optimize, qtables=qtables, restart_interval=ri,
                                        progressive=progressive) + (None,))[:3]                    # (Annex K: no tables come back)
    return _jpeg_files(x.shape[1], x.shape[2], quality, subsampling, segments, tables, qtables, ri, progressive)


def _jpeg_files(h, w, quality, subsampling, segments, tables, qtables, ri, progressive):
    """The files of images of one geometry and setting, from what _device_segments returns: around each image's segment(s) the
    header(s) that carry its `tables` - None: one header with the Annex K tables serves them all - and EOI."""
    if progressive:
        pieces = (jpeg_progressive_pieces(h, w, quality, subsampling, t, qtables=qtables, restart_interval=ri) for t in tables)
        return [b''.join(p + s for p, s in zip(front, ten)) + b'\xff\xd9' for front, ten in zip(pieces, segments)]
    heads = [_jpeg_header(h, w, quality, subsampling, None, qtables, ri)] * len(segments) if tables is None else \
        [_jpeg_header(h, w, quality, subsampling, t, qtables, ri) for t in tables]
    return [head + s + b'\xff\xd9' for head, s in zip(heads, segments)]


def _header_lengths(h, w, quality, subsampling, n, tables, qtables, ri, progressive):
    """The bytes _jpeg_files writes per image beside its segment(s) and EOI, a list of n: SOI .. SOS - 623, or 692 with three
    quantisation tables, a DRI segment counted, and with `tables` (n, 4, 272) each table's symbols in place of Annex K's 348 -, or
    everything in front of the ten scans of a progressive file."""
    if progressive:
        pieces = (jpeg_progressive_pieces(h, w, quality, subsampling, t, qtables=qtables, restart_interval=ri) for t in tables)
        return [sum(len(p) for p in front) for front in pieces]
    grey = ops.jpeg_is_grey(*_factors(subsampling))
    head = _header_bytes(qtables, ri, grey)[0]
    annex_k = _GREY_ANNEX_K_SYMBOLS if grey else _ANNEX_K_SYMBOLS
    return [head] * n if tables is None else (head - annex_k + tables[..., :16].sum(axis=(-2, -1), dtype=np.int64)).tolist()


def compress_batch(batch_x, jpeg_quality, effective=False, subsampling='4:4:4', optimize=False, *, qtables=None, restart_interval=0,
                   progressive=False):
    """Compress an image or a batch with the standard JPEG codec (jpeg_helpers.py:82-114).  (h,w,3) -> (float64 image, bytes);
    (n,h,w,3) -> (float32 batch, list of bytes).  `effective` counts from the first Huffman table on instead of the whole file.
    Every input, uint8 included, goes through the reference's conversion: x / 255 in float32 if the maximum exceeds 1, then
    (255 x) truncated - a byte k can come out as k - 1.  Values that numpy's cast would wrap are clamped to 0..255.
    `optimize`: the sizes are those of the files with optimised Huffman tables (encode_batch(optimize=True)); the image is the same.
    qtables (with jpeg_quality None, see check_qtables): the codec with these quantisation tables instead of a quality's; the sizes
    are those of encode_batch(qtables=) - a third table costs 69 bytes of header, none of the effective size.
    restart_interval: the sizes are those of encode_batch(restart_interval=), the DRI segment and the markers counted (both lie
    behind the first Huffman table, so `effective` counts them too); the image is the same.
    progressive: the sizes are those of encode_batch(progressive=True), `effective` again from the first Huffman table on (offset 177
    with two quantisation tables); the image is the same.
    (h,w,1) or (n,h,w,1): the grey-scale codec - the image comes back with its one channel, the sizes are those of
    encode_batch's grey-scale files, `effective` from the first Huffman table on (offset 102); subsampling left at its default or
    'grey', not with `progressive`."""
    grey = _grey_shape(np.shape(unwrap(batch_x)))
    subsampling = _grey_input(np.shape(unwrap(batch_x)), subsampling, 'compress_batch')           # ('grey' for such a shape, or refused)
    jpeg_quality, qtables = _quality_or_tables(jpeg_quality, qtables, grey=grey)
    ri = ops.jpeg_restart_interval(restart_interval)
    x = _device_batch(batch_x, keep_bytes=False)
    if x.dim() not in (3, 4):
        raise ValueError('compress_batch needs an (h,w,3) image or an (n,h,w,3) batch')
    single = x.dim() == 3
    image, segments, tables = (device_codec(x[None] if single else x, jpeg_quality, subsampling, optimize=optimize, qtables=qtables,
                                            restart_interval=ri, progressive=progressive) + (None,))[:3]
    heads = _header_lengths(x.shape[-3], x.shape[-2], jpeg_quality, subsampling, len(segments), tables, qtables, ri, progressive)
    dht = _header_bytes(qtables, ri, grey)[1] if effective else 0
    sizes = [head + (sum(len(scan) for scan in s) if progressive else len(s)) + 2 - dht for head, s in zip(heads, segments)]
    image = image.cpu().numpy()
    if single:
        return np.rint(image[0] * np.float32(255)).astype(np.uint8) / 255, sizes[0]
    return image, sizes


def match_quality(image, target=0.95, match='ssim', subsampling='4:4:4', optimize=False):
    """The JPEG quality 1..95 whose SSIM or bpp is closest to `target`, by the reference's bisection (jpeg_helpers.py:26-79); with
    `optimize` the bpp is that of the file with optimised Huffman tables."""
    from ..helpers import metrics
    assert image.ndim == 3, 'Only RGB images supported'
    _colour_only('match_quality', image.shape[-1] == 1)

    def ssim_gap(q):
        return metrics.ssim(image, compress_batch(image, q, subsampling=subsampling, optimize=optimize)[0].squeeze()) - target

    def bpp_gap(q):
        return 8 * np.mean(compress_batch(image, q, subsampling=subsampling, optimize=optimize)[1]) / image.shape[0] / image.shape[1] - target

    if match not in ('ssim', 'bpp'):
        raise ValueError('Invalid argument: match')
    gap = ssim_gap if match == 'ssim' else bpp_gap
    low, high = 1, 95
    gap_low, gap_high = gap(low), gap(high)
    while high - low > 1:
        if gap_low * gap_high > 0:
            raise ValueError('Same deviation for both end-points {} - {}'.format(low, high))
        mid = (low + high) // 2
        gap_mid = gap(mid)
        if gap_mid * gap_high > 0:
            high, gap_high = mid, gap_mid
        else:
            low, gap_low = mid, gap_mid
    return low if abs(gap_high) > abs(gap_low) else high


# ---- one quality per item --------------------------------------------------------------------------
RD_WORKSPACE_BUDGET = 2 << 30          # bytes of codec workspace one item call may take; a longer sweep is cut between qualities


def _check_qualities(qualities):
    q = np.asarray(qualities).reshape(-1)
    if q.size == 0 or not np.issubdtype(q.dtype, np.number) or (q != np.rint(q)).any() or q.min() < 1 or q.max() > 100:
        raise ValueError('Invalid JPEG qualities: {} (integers 1..100)'.format(list(np.asarray(qualities).reshape(-1))))
    return q.astype(np.int64)


def _file_bytes(lengths, effective, tables=None):
    head, dht = _header_bytes(tables)
    return head + lengths + 2 - (dht if effective else 0)


def _qualities_per_call(n, h, w, hs, vs, total):
    """How many qualities of a sweep over n images fit one item call: the workspace within RD_WORKSPACE_BUDGET (at least one)."""
    k = max(1, min(total, 65535 // n))
    while k > 1 and ops.jpeg_workspace_bytes(k * n, h, w, hs, vs) > RD_WORKSPACE_BUDGET:
        k -= 1
    return k


def _item_round(x, item_q, hs, vs, want_lengths, want_images, optimize=False, item_tables=None):
    """One item call: source batch x, one quality per item (item j = image j % n) -> (lengths (items,) int32 device tensor or None,
    decoded (items,h,w,3) device tensor or None).  Nothing is read back.  With `optimize` the lengths are those of the segments coded
    with each item's optimal tables plus what its header has beyond the 623 bytes (so that _file_bytes holds), and a third value is
    returned: the status (items,) int32 of JPEG_OPT_STATUS_BITS, or None.  item_tables (items, 3, 64): one table set per item on the
    device in place of the qualities (item_q is None then)."""
    _, h, w, _ = x.shape
    items = len(item_q) if item_tables is None else item_tables.shape[0]
    ws = torch.empty(ops.jpeg_workspace_bytes(items, h, w, hs, vs) or 1, dtype=torch.uint8, device=x.device)
    if item_tables is None:
        q = ops.jpeg_item_qualities(item_q, items, x.device)
        coef, _ = ops.jpeg_transform_items(x, q, hs, vs, workspace=ws)
    else:
        coef, _ = ops.jpeg_transform_tables(x, item_tables, hs, vs, workspace=ws)
    status = None
    if want_lengths and optimize:
        _, lengths, tables, status = _optimised(_coding(optimize=True), coef, h, w, hs, vs, 1)                # byte counts only
        lengths = lengths + (tables[:, :, :16].sum(dim=(1, 2), dtype=torch.int32) - 348)
    else:
        lengths = ops.jpeg_encode(coef, h, w, hs, vs, workspace=ws, capacity=1)[1] if want_lengths else None      # byte counts only
    y = None
    if want_images:
        y = ops.jpeg_reconstruct_items(coef, h, w, q, hs, vs, workspace=ws)[0] if item_tables is None else \
            ops.jpeg_reconstruct_tables(coef, h, w, item_tables, hs, vs, workspace=ws)
    return (lengths, y, status) if optimize else (lengths, y)


def rate_distortion(batch_x, qualities, subsampling='4:4:4', effective=True, want_images=False, optimize=False):
    """The rate-distortion table of a batch (n,h,w,3) over Q qualities: a dict of (Q, n) arrays 'ssim', 'psnr', 'msssim', 'msssim_db'
    (helpers.metrics of the source against what libjpeg decodes), 'bytes' and 'bpp' (compress_batch's count: the whole file, or from
    the first Huffman table on when `effective`).  With want_images also the decoded (Q,n,h,w,3) device tensor.  The batch is
    uploaded once and coded as Q * n items - one transform, one encode and one reconstruct call, or one set per group of qualities
    where the workspace would exceed RD_WORKSPACE_BUDGET - and the numbers come back in one download.  With `optimize` the byte counts
    are those of the files with optimised Huffman tables (three more calls per group); everything else is unchanged."""
    q = _check_qualities(qualities)
    hs, vs = ops.jpeg_subsampling(subsampling)
    x = _device_batch(batch_x, keep_bytes=False)
    _colour_only('rate_distortion', x.dim() == 4 and x.shape[3] == 1)
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError('rate_distortion needs an (n,h,w,3) batch')
    n = x.shape[0]
    # quality-major: item j = (part[j // n], image j % n)
    return _rate_distortion(x, len(q), hs, vs, lambda k0, k1: _item_round(x, np.repeat(q[k0:k1], n), hs, vs, True, True, optimize),
                            effective, want_images, optimize, None)


def _rate_distortion(x, total, hs, vs, item_round, effective, want_images, optimize, tables):
    """The table of rate_distortion over `total` rows (qualities or table sets) of the device batch x: item_round(k0, k1) codes rows
    k0 .. k1 - 1 as (k1 - k0) * n items, row-major, and returns what _item_round does; `tables` is what _file_bytes counts the
    header from."""
    from ..helpers import metrics
    n, h, w, _ = x.shape
    step = _qualities_per_call(n, h, w, hs, vs, total)
    rows, images = [], []
    for k0 in range(0, total, step):
        part = range(k0, min(k0 + step, total))
        done = item_round(part.start, part.stop)
        lengths, y = done[0], done[1]
        status = done[2] if optimize else torch.zeros_like(lengths)
        y = y.view(len(part), n, h, w, 3)
        for k in range(len(part)):
            ms = metrics._msssim_device(x, y[k])
            rows.append(torch.stack([ops.ssim(x, y[k], mode='skimage', max_val=1.0).double(),
                                     10.0 * torch.log10(1.0 / metrics._mean_per_image(x, y[k], lambda d: d * d)),
                                     torch.full((n,), float('nan'), dtype=torch.float64, device=x.device) if ms is None else ms.double(),
                                     lengths[k * n:(k + 1) * n].double(), status[k * n:(k + 1) * n].double()]))
        if want_images:
            images.append(y)
    table = torch.stack(rows).cpu().numpy()                            # (Q, 5, n): the one download
    _raise_on_opt_status(table[:, 4].astype(np.int64).reshape(-1))
    size = _file_bytes(table[:, 3].astype(np.int64), effective, tables)
    with np.errstate(divide='ignore'):
        out = {'ssim': table[:, 0], 'psnr': table[:, 1], 'msssim': table[:, 2], 'msssim_db': -10.0 * np.log10(1.0 - table[:, 2]),
               'bytes': size, 'bpp': 8 * size / h / w}
    if want_images:
        return out, (images[0] if len(images) == 1 else torch.cat(images))
    return out


def rate_distortion_tables(batch_x, tables, subsampling='4:4:4', effective=True, want_images=False, optimize=False):
    """rate_distortion over K quantisation table sets in place of qualities: tables (K, T, 64) or (K, T, 8, 8), T = 2 or 3, every set
    as check_qtables takes it - a quality ladder of learned tables, say.  Returns the dictionary of rate_distortion with (K, n)
    arrays (the byte counts those of compress_batch(qtables=tables[k])), with want_images also the decoded (K,n,h,w,3) device tensor.
    The batch is coded as K * n items, one table set per item, in one transform, one encode and one reconstruct call per group
    within RD_WORKSPACE_BUDGET, and the numbers come back in one download."""
    if np.ndim(tables) not in (3, 4) or len(tables) == 0:
        raise ValueError('rate_distortion_tables: table sets (K, T, 64) or (K, T, 8, 8) needed, got shape {}'.format(np.shape(tables)))
    sets = np.stack([check_qtables(t) for t in tables])
    hs, vs = ops.jpeg_subsampling(subsampling)
    x = _device_batch(batch_x, keep_bytes=False)
    _colour_only('rate_distortion_tables', x.dim() == 4 and x.shape[3] == 1)
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError('rate_distortion_tables needs an (n,h,w,3) batch')
    n = x.shape[0]
    # set-major: item j = (sets[j // n], image j % n)
    return _rate_distortion(x, len(sets), hs, vs,
                            lambda k0, k1: _item_round(x, None, hs, vs, True, True, optimize, _device_tables(sets[k0:k1], n, x.device)),
                            effective, want_images, optimize, sets[0])


def match_quality_batch(batch_x, target=0.95, match='ssim', subsampling='4:4:4', optimize=False):
    """match_quality for every image of a batch (n,h,w,3) at once: the reference's bisection over 1..95, where each round is one item
    call in which image i carries its own current quality - 8 calls whatever n is (the two end points share the first).  `target`
    is a scalar or one value per image.  Returns an int array (n,).  An image whose end points do not bracket its target raises the
    reference's ValueError, naming the first such image.  With `optimize` the bpp is that of the files with optimised Huffman tables."""
    if match not in ('ssim', 'bpp'):
        raise ValueError('Invalid argument: match')
    shape = tuple(unwrap(batch_x).shape)
    _colour_only('match_quality_batch', len(shape) == 4 and shape[3] == 1)
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError('match_quality_batch needs an (n,h,w,3) batch')
    n, h, w, _ = shape
    target = np.asarray(target, dtype=np.float64)
    if target.ndim > 1 or (target.ndim == 1 and len(target) != n):
        raise ValueError('target: a scalar or {} values needed, got shape {}'.format(n, target.shape))
    target = np.broadcast_to(target, (n,))
    hs, vs = ops.jpeg_subsampling(subsampling)
    x = _device_batch(batch_x, keep_bytes=False)

    def gaps(item_q):            # item j = image j % n at item_q[j] -> its gap to the target, as match_quality's ssim_gap / bpp_gap
        reps = len(item_q) // n
        if match == 'ssim':
            _, y = _item_round(x, item_q, hs, vs, False, True)
            v = torch.cat([ops.ssim(x, y[r * n:(r + 1) * n], mode='skimage', max_val=1.0) for r in range(reps)]).double().cpu().numpy()
        else:
            if optimize:
                lengths, _, status = _item_round(x, item_q, hs, vs, True, False, True)
                lengths, status = torch.stack([lengths, status]).cpu().numpy()
                _raise_on_opt_status(status)
            else:
                lengths = _item_round(x, item_q, hs, vs, True, False)[0].cpu().numpy()
            v = 8 * _file_bytes(lengths.astype(np.float64), False) / h / w
        return v - np.tile(target, reps)

    low, high = np.full(n, 1, np.int64), np.full(n, 95, np.int64)
    ends = gaps(np.concatenate([low, high]))
    gap_low, gap_high = ends[:n].copy(), ends[n:].copy()
    while (high - low > 1).any():
        active = high - low > 1
        same = active & (gap_low * gap_high > 0)
        if same.any():
            i = int(np.flatnonzero(same)[0])
            raise ValueError('Same deviation for both end-points {} - {} (image {})'.format(low[i], high[i], i))
        mid = np.where(active, (low + high) // 2, low)               # a finished image rides along at a quality it has seen
        gap_mid = gaps(mid)
        up = active & (gap_mid * gap_high > 0)
        down = active & ~up
        high[up], gap_high[up] = mid[up], gap_mid[up]
        low[down], gap_low[down] = mid[down], gap_mid[down]
    return np.where(np.abs(gap_high) > np.abs(gap_low), low, high)


# ---- reading files ---------------------------------------------------------------------------------
class JPEGHeader(namedtuple('JPEGHeader', 'h w hs vs qtables huffman ecd_offset ecd_end restart_interval', defaults=(0,))):
    """parse_header's result.  The tuple keeps the nine fields it had before progressive files were read (callers unpack it and count
    on restart_interval as its last); `scans` - a JPEGScan per scan of a progressive file, () for a baseline file - is an attribute
    next to them, set by with_scans.  So is `ncomp`, the components of the frame: 3, or 1 for a grey-scale file (allow_grey), whose
    qtables are (1, 64) and whose huffman holds two pairs."""
    scans = ()
    ncomp = 3

    def with_scans(self, scans):
        out = self._replace()
        out.scans, out.ncomp = tuple(scans), self.ncomp
        return out

    def with_ncomp(self, ncomp):
        out = self._replace()
        out.scans, out.ncomp = self.scans, int(ncomp)
        return out


# one scan of a progressive file: components (indices in frame order), the band and the bit positions of its SOS segment, huffman = the
# (16 counts, symbols) table of each component of the scan (empty for a DC refine scan, which has no symbols), and where its
# entropy-coded segment stands in the file
JPEGScan = namedtuple('JPEGScan', 'components ss se ah al huffman ecd_offset ecd_end')
_NO_TABLE = (bytes(16), b'')          # the table of a scan that has no symbols, and of the slots of a scan that its components leave free
# what a reader takes beyond baseline colour files of the three standard samplings: the allow_* answers of its caller, in parse_header's order
_Accept = namedtuple('_Accept', 'restart progressive grey sampling')
JPEG_SCANS_MAX = ops.JPEG_SCANS_MAX
JPEG_STATUS_BITS = OrderedDict([(1, 'marker inside the entropy-coded segment'), (2, 'invalid Huffman code'), (4, 'zig-zag index past 63'),
                                (8, 'coefficient category out of range'), (16, 'bits needed beyond the end of the stream'),
                                (32, 'fewer blocks than the scan has'), (64, 'DC value outside int16'),
                                (128, 'Huffman table that is no prefix code'), (256, 'bad segment offsets'),
                                (512, 'restart markers missing, surplus or out of sequence'),
                                (1024, 'end-of-band run beyond the blocks of the scan')])
_MAX_SIDE = 4096
_NATURAL = np.argsort(zigzag(8).ravel(), kind='stable')                  # scan position -> natural index, as a DQT segment is read
_SOF_NAMES = {0xc1: 'extended sequential', 0xc2: 'progressive', 0xc3: 'lossless', 0xc5: 'differential sequential',
              0xc6: 'differential progressive', 0xc7: 'differential lossless', 0xc9: 'arithmetic-coded sequential',
              0xca: 'arithmetic-coded progressive', 0xcb: 'arithmetic-coded lossless', 0xcd: 'arithmetic-coded differential sequential',
              0xce: 'arithmetic-coded differential progressive', 0xcf: 'arithmetic-coded differential lossless'}


def parse_header(data, allow_restart=False, allow_progressive=False, allow_grey=False, allow_sampling=False):
    """The header of a baseline JPEG file, read on the host without decoding: JPEGHeader(h, w, hs, vs, qtables (3, 64) uint16 in
    natural order per component, huffman = six (16 counts, symbols) pairs of bytes in the order Y-DC, Y-AC, Cb-DC, Cb-AC, Cr-DC, Cr-AC
    as the DHT bodies have them, ecd_offset, ecd_end = the offset of the final FFD9, restart_interval).  Accepted: SOF0 with 8-bit
    samples, three components in one interleaved scan, luma sampling 1x1, 2x1 or 2x2 over 1x1 chroma, any 8-bit quantisation and any
    Huffman tables in any assignment, no restart interval; APPn and COM are skipped.  Every other file raises ValueError naming the
    reason.  allow_restart: a file with a restart interval (a DRI segment with a value above 0) is accepted
    too - restart_interval is that value in MCUs, and the markers FFD0 .. FFD7 in the entropy-coded segment are stepped over (their
    number and sequence are the decoder's to check, status bit 512).  Still refused: a restart marker in a file whose interval is 0,
    and several DRI segments with different values (libjpeg would let the last one hold).  allow_progressive: a progressive file
    (SOF2, Huffman-coded, 8-bit samples, three components, the samplings above) is accepted too, with any legal scan script (DESIGN.md
    section 4n).  All its scans are walked: `scans` holds one JPEGScan per scan with the tables in force at its SOS, `huffman` is (),
    ecd_offset / ecd_end span the first scan to the final FFD9.  Refused by name: a script that breaks T.81's rules or leaves a
    coefficient short of Al = 0, a restart interval that changes between scans, more than 64 scans, a DNL marker, a missing table,
    any marker between scans but DHT, DRI, COM and APPn.  allow_grey: a grey-scale file - a frame of one
    component, SOF0 or with allow_progressive SOF2, 8-bit samples, every scan of that component, any Huffman table ids, with
    allow_restart a DRI - is accepted too.  Its sampling factors may be any of 1..4: a one-component scan is never interleaved, so they
    change nothing, and hs = vs = 1 is reported.  Its qtables are (1, 64), its huffman two pairs (DC, AC), its `ncomp` 1.
    allow_sampling: a colour file whose luma sampling is 1x2 (4:4:0), 4x1 (4:1:1), 4x2 (4:1:0), 1x4 or 2x4 over 1x1 chroma (DESIGN.md
    section 4r) is accepted too, baseline or with allow_progressive progressive, with allow_restart a DRI.  Still refused, the factors
    named: chroma that is not 1x1, a factor of 3, and every pair whose ratios are not those (4x4, ...)."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError('JPEG data: bytes needed, got {}'.format(type(data).__name__))
    accept = _Accept(allow_restart, allow_progressive, allow_grey, allow_sampling)
    data = bytes(data)
    if data[:2] != b'\xff\xd8':
        raise ValueError('not a JPEG file: no SOI marker')
    qt, huff, frame, pos, restart, progressive = {}, {}, None, 2, None, False
    while True:
        if pos + 4 > len(data):
            raise ValueError('truncated file: no SOS marker')
        if data[pos] != 0xff:
            raise ValueError('no marker at offset {}'.format(pos))
        marker = data[pos + 1]
        if marker == 0xff:                                               # fill byte
            pos += 1
            continue
        if marker == 0xd9:
            raise ValueError('EOI before any scan')
        if marker == 0xd8 or marker == 0x01 or 0xd0 <= marker <= 0xd7:
            raise ValueError('unexpected marker FF{:02X} in the header'.format(marker))
        marker, body, pos = _segment(data, pos)
        if marker == 0xdb:
            k = 0
            while k < len(body):
                if body[k] >> 4:
                    raise ValueError('16-bit quantisation table (DQT precision {})'.format(body[k] >> 4))
                if (body[k] & 15) > 3 or k + 65 > len(body):
                    raise ValueError('malformed DQT segment')
                table = np.zeros(64, np.uint16)
                table[_NATURAL] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                qt[body[k] & 15] = table
                k += 65
        elif marker == 0xc4:
            huff.update(_dht_tables(body))
        elif marker == 0xc0 or (marker == 0xc2 and accept.progressive):
            progressive = marker == 0xc2
            if frame is not None:
                raise ValueError('several frame headers')
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError('malformed SOF0 segment')
            if body[0] != 8:
                raise ValueError('{}-bit samples (only 8-bit baseline files are read)'.format(body[0]))
            h, w, ncomp = struct.unpack_from('>HH', body, 1) + (body[5],)
            if ncomp != 3 and not (ncomp == 1 and accept.grey):
                raise ValueError('{} (3 components needed, the file has {})'.format(
                    {1: 'grey-scale file', 4: 'CMYK / four-component file'}.get(ncomp, 'unsupported number of components'), ncomp))
            if h < 1 or w < 1 or h > _MAX_SIDE or w > _MAX_SIDE:
                raise ValueError('unsupported size {}x{} (1..{} per side)'.format(h, w, _MAX_SIDE))
            comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(ncomp)]
            sampling = tuple(c[1:3] for c in comps)
            if ncomp == 1:
                if not (1 <= sampling[0][0] <= 4 and 1 <= sampling[0][1] <= 4):
                    raise ValueError('illegal sampling factors {}x{} of the one component (1..4 each)'.format(*sampling[0]))
            elif sampling[1:] != ((1, 1), (1, 1)) or not (sampling[0] in ops.JPEG_SUBSAMPLING.values()
                                                          or (accept.sampling and ops.jpeg_is_wide(*sampling[0]))):
                raise ValueError('unsupported sampling factors {} (luma {} over 1x1 chroma)'.format(
                    ' '.join('{}x{}'.format(*f) for f in sampling),
                    '1x1, 2x1, 2x2, 1x2, 4x1, 4x2, 1x4 or 2x4' if accept.sampling else '1x1, 2x1 or 2x2'))
            frame = (h, w, comps)
        elif marker in _SOF_NAMES:
            raise ValueError('{} file (SOF{}): only baseline sequential files (SOF0) are read'.format(_SOF_NAMES[marker], marker - 0xc0))
        elif marker == 0xcc:
            raise ValueError('arithmetic-coded file (DAC segment)')
        elif marker == 0xdd:
            value = _dri_value(body)
            if value != 0 and not accept.restart:
                raise ValueError('restart interval {} (DRI): files with restart markers are not read'.format(value))
            if restart is not None and restart != value:
                raise ValueError('several DRI segments with different restart intervals ({} and {}; libjpeg lets the last one hold): '
                                 'not read'.format(restart, value))
            restart = value
        elif marker == 0xda:
            break
        elif not (0xe0 <= marker <= 0xef or marker == 0xfe or marker == 0xdc or 0xf0 <= marker <= 0xfd):
            raise ValueError('unsupported marker FF{:02X} in the header'.format(marker))
    if frame is None:
        raise ValueError('no frame header (SOF0) before the scan')
    scans = _progressive_scans if progressive else _baseline_scan         # from the first SOS segment's body and the offset behind it
    return scans(data, body, pos, frame, qt, huff, restart or 0, accept)


def _segment(data, pos):
    """The marker segment at pos -> (marker, body, the offset behind it).  That there are four bytes at pos is the caller's to see."""
    marker, size = data[pos + 1], struct.unpack_from('>H', data, pos + 2)[0]
    if size < 2 or pos + 2 + size > len(data):
        raise ValueError('truncated segment FF{:02X} at offset {}'.format(marker, pos))
    return marker, data[pos + 4:pos + 2 + size], pos + 2 + size


def _sos_fields(body):
    """The body of an SOS segment -> (component ids, their table selectors Td << 4 | Ta, Ss, Se, Ah, Al)."""
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise ValueError('malformed SOS segment')
    ns = body[0]
    return list(body[1:1 + 2 * ns:2]), list(body[2:2 + 2 * ns:2]), body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15


def _dri_value(body):
    if len(body) != 2:
        raise ValueError('malformed DRI segment')
    return struct.unpack('>H', body)[0]


def _huffman_tables(huff, selector, c, classes, where=''):
    """The tables of `classes` (0 DC, 1 AC) that a scan's selector names for component c, of the tables `huff` in force at its SOS."""
    if (selector >> 4) > 3 or (selector & 15) > 3:
        raise ValueError('malformed SOS segment')
    keys = [cls << 4 | (selector & 15 if cls else selector >> 4) for cls in classes]
    for key in keys:
        if key not in huff:
            raise ValueError('missing Huffman table: {} table {} of component {}{}'.format('AC' if key >> 4 else 'DC', key & 15, c, where))
    return [huff[key] for key in keys]


def _qtable(qt, comps, c):
    if comps[c][3] not in qt:
        raise ValueError('missing quantisation table {} of component {}'.format(comps[c][3], c))
    return qt[comps[c][3]]


def _header(frame, qtables, huffman, ecd_offset, ecd_end, restart, scans=()):
    """parse_header's result.  The scans of one component are never interleaved, so its sampling factors change nothing: 1x1."""
    h, w, comps = frame
    hs, vs = (1, 1) if len(comps) == 1 else comps[0][1:3]
    return JPEGHeader(h, w, hs, vs, np.stack(qtables), huffman, ecd_offset, ecd_end, restart).with_ncomp(len(comps)).with_scans(scans)


_NOT_STUFFED = re.compile(b'\xff[^\\x00]')          # FF and a second byte that is not the 00 stuffed behind a data FF


def _segment_end(data, k, restart, allow_restart, fill=True):
    """The offset of the first marker behind the entropy-coded segment that starts at k; restart markers are stepped over.  So are,
    with `fill`, the fill bytes in front of that marker (FF FF ..), which then count into the segment - as in the scans of a
    progressive file; without it the segment ends at the first of them, for the caller to refuse."""
    while True:
        found = _NOT_STUFFED.search(data, k)
        if found is None:
            raise ValueError('no EOI marker behind the entropy-coded segment')
        k = found.start()
        nxt = data[k + 1]
        if 0xd0 <= nxt <= 0xd7:
            if not allow_restart:
                raise ValueError('restart marker FF{:02X} in the entropy-coded segment: files with restart markers are not read'.format(nxt))
            if not restart:
                raise ValueError('restart marker FF{:02X} in the entropy-coded segment of a file whose restart interval is 0'.format(nxt))
            k += 2
        elif nxt == 0xff and fill:
            k += 1
        else:
            return k


def _baseline_scan(data, body, start, frame, qt, huff, restart, accept):
    """The one scan of a baseline file, whose SOS body is `body` and whose entropy-coded segment starts at `start` -> its JPEGHeader."""
    comps = frame[2]
    ids, selectors, ss, se, ah, al = _sos_fields(body)
    if len(comps) == 1 and len(ids) != 1:
        raise ValueError('the scan holds {} components, the frame of a grey-scale file one'.format(len(ids)))
    if len(ids) != len(comps):
        raise ValueError('non-interleaved file: the scan holds {} of 3 components'.format(len(ids)))
    if ids != [c[0] for c in comps]:
        raise ValueError('the scan does not list the components in frame order')
    if (ss, se, ah, al) != (0, 63, 0, 0):
        raise ValueError('not a baseline scan: Ss={} Se={} Ah/Al={:02x} (0, 63, 00 needed)'.format(ss, se, ah << 4 | al))
    tables, qtables = [], []
    for c, selector in enumerate(selectors):                            # (a component's Huffman tables are missed before its quantisation table)
        tables += _huffman_tables(huff, selector, c, (0, 1))
        qtables.append(_qtable(qt, comps, c))
    end = _segment_end(data, start, restart, accept.restart, fill=False)
    if data[end + 1] in (0xda, 0xc4, 0xdb, 0xdd):
        raise ValueError('several scans: marker FF{:02X} behind the first entropy-coded segment'.format(data[end + 1]))
    if data[end + 1] != 0xd9:                                            # a fill byte (FFFF) too: the decoder is never given one
        raise ValueError('unexpected marker FF{:02X} in the entropy-coded segment'.format(data[end + 1]))
    return _header(frame, qtables, tuple(tables), start, end, restart)


def jpeg_script_check(script, ncomp=3):
    """script: [(components, Ss, Se, Ah, Al)] -> the level of every scan (1 + the highest level of an earlier
    scan of a shared component whose band overlaps); ValueError names the rule of T.81 G.1.1.1 a script breaks.  ncomp: the components
    of the frame, 3 or 1 - every scan of a grey-scale file holds its one component."""
    if len(script) > JPEG_SCANS_MAX:
        raise ValueError('progressive file with {} scans (at most {} are read)'.format(len(script), JPEG_SCANS_MAX))
    al_of, levels = [[None] * 64 for _ in range(ncomp)], []
    for i, (cs, ss, se, ah, al) in enumerate(script):
        where = 'scan {} (components {} Ss={} Se={} Ah={} Al={})'.format(i, list(cs), ss, se, ah, al)
        if ss == 0 and se != 0:
            raise ValueError('illegal progressive script: {} mixes DC and AC coefficients'.format(where))
        if ss > se or se > 63 or ah > 13 or al > 13:
            raise ValueError('illegal progressive script: {} has a band or bit position out of range'.format(where))
        if ncomp == 1 and tuple(cs) != (0,):
            raise ValueError('illegal progressive script: {} - every scan of a one-component frame holds that component, once'.format(where))
        if tuple(cs) not in ((0,), (1,), (2,), (0, 1, 2)) or (ss > 0 and len(cs) != 1):
            raise ValueError('illegal progressive script: {} - a DC scan holds one component or all three in frame order, an AC scan '
                             'exactly one'.format(where))
        for c in cs:
            if ss > 0 and al_of[c][0] is None:
                raise ValueError('illegal progressive script: {} comes before the DC first scan of its component'.format(where))
            for k in range(ss, se + 1):
                if (al_of[c][k] is not None) if ah == 0 else (al_of[c][k] != ah or al != ah - 1):
                    raise ValueError('illegal progressive script: {} - a first scan has Ah = 0 and is the first of its coefficients, a '
                                     'refinement has Ah = the Al before it and Al = Ah - 1'.format(where))
                al_of[c][k] = al
        levels.append(1 + max([lv for lv, (ce, se0, se1, _, _) in zip(levels, script) if set(ce) & set(cs) and se0 <= se and ss <= se1]
                              or [0]))
    short = [(c, k) for c in range(ncomp) for k in range(64) if al_of[c][k] != 0]
    if short:
        raise ValueError('incomplete progression: coefficient {} of component {} never reaches Al = 0 ({} such coefficients; libjpeg '
                         'smooths such files)'.format(short[0][1], short[0][0], len(short)))
    return levels


def _progressive_scans(data, body, start, frame, qt, huff, restart, accept):
    """The scans of a progressive file, the first with the SOS body `body` and its entropy-coded segment at `start` -> its JPEGHeader."""
    comps = frame[2]
    ids, huff, scans = [c[0] for c in comps], dict(huff), []
    while True:
        listed, selectors, ss, se, ah, al = _sos_fields(body)
        if len(scans) == JPEG_SCANS_MAX:
            raise ValueError('progressive file with more than {} scans'.format(JPEG_SCANS_MAX))
        if any(i not in ids for i in listed):
            raise ValueError('malformed SOS segment: unknown component')
        cs = tuple(ids.index(i) for i in listed)
        classes = () if ss == 0 and ah else (int(ss > 0),)             # a DC refine scan has no symbols; else the DC or the AC table
        where = ' in scan {}'.format(len(scans))
        tables = tuple(t for c, selector in zip(cs, selectors)
                       for t in _huffman_tables(huff, selector, c, classes, where) or [_NO_TABLE])
        pos = _segment_end(data, start, restart, accept.restart)
        scans.append(JPEGScan(cs, ss, se, ah, al, tables, start, pos))
        while data[pos + 1] != 0xd9:                                     # the markers between two scans
            if pos + 4 > len(data):
                raise ValueError('truncated file behind scan {}'.format(len(scans) - 1))
            marker, body, behind = _segment(data, pos)
            if marker == 0xda:
                start = behind
                break
            if marker == 0xc4:
                huff.update(_dht_tables(body))
            elif marker == 0xdd:
                value = _dri_value(body)
                if value != restart:
                    raise ValueError('the restart interval changes between scans ({} then {}): not read'.format(restart, value))
            elif marker == 0xdc:
                raise ValueError('DNL marker behind scan {}: not read'.format(len(scans) - 1))
            elif not (0xe0 <= marker <= 0xef or marker == 0xfe):
                raise ValueError('unsupported marker FF{:02X} between the scans of a progressive file'.format(marker))
            pos = behind
            while pos + 1 < len(data) and data[pos] == 0xff and data[pos + 1] == 0xff:          # fill bytes
                pos += 1
            if pos + 1 >= len(data):
                raise ValueError('truncated file behind scan {}: no EOI marker'.format(len(scans) - 1))
            if data[pos] != 0xff:
                raise ValueError('no marker at offset {}'.format(pos))
        if data[pos + 1] == 0xd9:
            break
    jpeg_script_check([s[:5] for s in scans], len(comps))
    return _header(frame, [_qtable(qt, comps, c) for c in range(len(comps))], (), scans[0].ecd_offset, pos, restart, scans)


def _dht_tables(body):
    """The tables of one DHT segment: {Tc << 4 | Th: (16 counts, symbols)}."""
    out, k = {}, 0
    while k < len(body):
        if k + 17 > len(body) or (body[k] >> 4) > 1 or (body[k] & 15) > 3:
            raise ValueError('malformed DHT segment')
        count = sum(body[k + 1:k + 17])
        if count > 256 or k + 17 + count > len(body):
            raise ValueError('malformed DHT segment')
        out[body[k]] = (bytes(body[k + 1:k + 17]), bytes(body[k + 17:k + 17 + count]))
        k += 17 + count
    return out


def _status_text(status):
    return ' | '.join(text for bit, text in JPEG_STATUS_BITS.items() if status & bit)


class _Group(namedtuple('_Group', 'indices h w hs vs restart_interval script coef status rounds qtabs')):
    """The files of one decode call (_decode_groups): their indices in the input, what they share - (hs, vs) = ops.JPEG_GREY for
    grey-scale files, script = () for baseline ones - and what is on the device for them; qtabs (n, 3 | 1, 64) went up with the files."""

    @property
    def geometry(self):
        return self.h, self.w, self.hs, self.vs


def _decode_groups(files, subseq_bits, device, accept, headers=None):
    """Headers parsed, one upload, one nimg_jpeg_decode[_restart] per group of equal (h, w, hs, vs, restart interval) - for progressive
    files (accept.progressive) one nimg_jpeg_decode_progressive per group of equal geometry, interval and scan script.  Returns
    (headers, [_Group]) - device tensors, nothing read back.  The (hs, vs) of a group of grey-scale files (accept.grey) is
    ops.JPEG_GREY: another geometry, so never in a group with colour files.  `headers`: the files' headers, where the caller has
    parsed them already."""
    headers = [parse_header(f, *accept) for f in files] if headers is None else headers
    if not headers:
        raise ValueError('no files to decode')
    keys = OrderedDict()
    for i, hd in enumerate(headers):
        hs, vs = ops.JPEG_GREY if hd.ncomp == 1 else (hd.hs, hd.vs)
        keys.setdefault((hd.h, hd.w, hs, vs, hd.restart_interval, tuple(s[:5] for s in hd.scans)), []).append(i)
    dev = device if device is not None else default_device()
    # what goes up, per group and back to back in group order: the segments - one per file or one per scan, a header standing for its
    # one scan -, their Huffman tables - six per file (grey: two), or three per scan - and three quantisation tables per file, or one
    segments = [[files[i][s.ecd_offset:s.ecd_end] for i in idx for s in headers[i].scans or (headers[i],)] for idx in keys.values()]
    tables = [[t for i in idx for s in headers[i].scans or (headers[i],)
               for t in (s.huffman + (_NO_TABLE,) * (3 - len(s.huffman)) if headers[i].scans else s.huffman)] for idx in keys.values()]
    qtabs = [np.stack([headers[i].qtables for i in idx]) for idx in keys.values()]
    blob = b''.join(s for group in segments for s in group)
    huff = np.zeros((sum(len(group) for group in tables), 272), np.uint8)
    for j, (counts, symbols) in enumerate(t for group in tables for t in group):
        huff[j, :16] = np.frombuffer(counts, np.uint8)
        huff[j, 16:16 + len(symbols)] = np.frombuffer(symbols, np.uint8)
    ecd = torch.from_numpy(np.frombuffer(blob if blob else b'\0', np.uint8).copy()).to(dev)
    huff = torch.from_numpy(huff).to(dev)
    qt = torch.from_numpy(np.concatenate([q.reshape(-1) for q in qtabs]).view(np.int16)).to(dev)
    b, t, q = (np.concatenate([[0], np.cumsum(sizes)]) for sizes in ([sum(len(s) for s in group) for group in segments],
                                                                   [len(group) for group in tables], [x.size for x in qtabs]))
    groups = []
    for g, ((h, w, hs, vs, ri, script), idx) in enumerate(keys.items()):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in segments[g]])]).astype(np.int64)).to(dev)
        part = ecd[b[g]:max(b[g + 1], b[g] + 1)]
        if script:
            rows = np.array([[sum(1 << c for c in cs), ss, se, ah, al, lv]
                             for (cs, ss, se, ah, al), lv in zip(script, jpeg_script_check(script, qtabs[g].shape[1]))], np.int32)
            done = ops.jpeg_decode_progressive(part, off, huff[t[g]:t[g + 1]].view(len(idx), len(script), 3, 272), rows, h, w, hs, vs,
                                               subseq_bits=subseq_bits, restart_interval=ri)
        else:
            done = ops.jpeg_decode(part, off, huff[t[g]:t[g + 1]].view(len(idx), -1, 272), h, w, hs, vs, subseq_bits=subseq_bits,
                                   restart_interval=ri)
        groups.append(_Group(idx, h, w, hs, vs, ri, script, *done, qt[q[g]:q[g + 1]].view(qtabs[g].shape)))
    return headers, groups


def _raise_on_status(groups, status):
    """status: numpy per group, in group order."""
    bad = sorted((i, int(s)) for g, st in zip(groups, status) for i, s in zip(g.indices, st) if s)
    if bad:
        raise ValueError('damaged JPEG data in file(s) {}: {}'.format(
            [i for i, _ in bad], '; '.join('{}: status {} ({})'.format(i, s, _status_text(s)) for i, s in bad)))


def _fetch_status(groups, more=()):
    """The one download of a reader: the status words of every group and behind them the device tensors `more` (uint8 or float32), in a
    single copy.  Damaged data raises (_raise_on_status); returns `more` as numpy arrays."""
    words = [len(g.indices) for g in groups]
    flat = torch.cat([g.status.view(torch.uint8) for g in groups] + [y.view(torch.uint8).reshape(-1) for y in more]).cpu().numpy()
    ends = np.cumsum([4 * sum(words)] + [y.numel() * y.element_size() for y in more])
    _raise_on_status(groups, np.split(flat[:ends[0]].view(np.int32), np.cumsum(words)[:-1]))
    return [flat[lo:hi].view(np.float32 if y.dtype == torch.float32 else np.uint8).reshape(tuple(y.shape))
            for y, lo, hi in zip(more, ends[:-1], ends[1:])]


def _as_files(files):
    """One file or several -> a list of bytes."""
    return [bytes(files)] if isinstance(files, (bytes, bytearray, memoryview)) else [bytes(f) for f in files]


def scaled_size(h, w, scale):
    """(rows, cols) of an h x w file decoded with decode_batch(scale=): ceil(h / scale), ceil(w / scale), as libjpeg rounds."""
    return ops.jpeg_scaled_size(h, w, scale)


def draft_scale(h, w, size):
    """The scale Pillow's Image.draft(mode, size) chooses for an h x w file and a requested size (width, height): the largest of 8, 4,
    2, 1 that is not above min(w // size[0], h // size[1]) - the image stays at least as large as asked for - and 1 where that is 0."""
    ratio = min(w // int(size[0]), h // int(size[1]))
    return next((s for s in (8, 4, 2) if s <= ratio), 1)


def decode_batch(files, as_float=False, device_output=False, subseq_bits=0, device=None, *, allow_restart=False, allow_progressive=False,
                 allow_grey=False, allow_sampling=False, scale=1):
    """Decode baseline JPEG files on the GPU: a list of bytes (or one bytes) -> (n,h,w,3) uint8, the array imageio.imread returns for
    each (libjpeg's islow inverse DCT and fancy up-sampling, bit for bit), or float32(byte) / 255 with as_float.  Files of different
    geometry give a list of (h,w,3) arrays in input order.  Any 8-bit quantisation and Huffman tables are read from each file
    (parse_header names what is refused).  The segments go up in one copy, every group of equal (h, w, sampling) takes one decode and
    one reconstruct call, status and images come down once; device_output keeps the images on the device.  Damaged data raises
    ValueError naming the indices and the status bits (JPEG_STATUS_BITS).  allow_restart: files with a restart interval are read
    too (parse_header); a group is then the files of equal geometry and interval, and every interval is decoded from its own start.
    allow_progressive: progressive files of any legal scan script are read too (parse_header), next to baseline
    ones in the same call; a group is then the files of equal geometry, interval and script (nimg_jpeg_decode_progressive).
    allow_grey: grey-scale files are read too (parse_header) and decode to (n,h,w,1) - the array imageio.imread
    returns for them with a last axis added; next to colour files they are another geometry, so the result is then a list.
    allow_sampling: colour files of the samplings 4:4:0, 4:1:1, 4:1:0, 1x4 and 2x4 are read too (parse_header), at
    every scale, with the up-sampling libjpeg chooses for them; a sampling is part of the geometry, as it always was.
    scale (1, 2, 4 or 8): every file is decoded at 1 / scale, to (n, ceil(h / scale), ceil(w / scale), 3 | 1) -
    libjpeg's scaled decoding, the pixels Pillow returns after Image.draft() (draft_scale names the scale it chooses), by reduced
    inverse DCTs in place of the full one (ops.jpeg_reconstruct_scaled); the entropy decoding is the same.  At a reduced scale the files
    of ONE geometry come back as one batch in input order whatever their restart intervals and scan scripts (at scale 1 they stay the
    list they were).  Any other scale is a ValueError before a byte goes to the device."""
    scale = ops.jpeg_scale(scale)
    files = _as_files(files)
    _, groups = _decode_groups(files, subseq_bits, device, _Accept(allow_restart, allow_progressive, allow_grey, allow_sampling))
    if scale == 1:
        images = [ops.jpeg_reconstruct_tables(g.coef, g.h, g.w, g.qtabs, g.hs, g.vs, out_u8=not as_float) for g in groups]
    else:
        images = [ops.jpeg_reconstruct_scaled(g.coef, g.h, g.w, g.qtabs, scale, g.hs, g.vs, out_u8=not as_float) for g in groups]
    fetched = _fetch_status(groups, () if device_output else images)    # one download: the status words, then the images
    images = images if device_output else fetched
    if len(groups) == 1:
        return images[0]
    if scale != 1 and len({g.geometry for g in groups}) == 1:           # one geometry, several intervals or scripts: one batch
        order = np.argsort([i for g in groups for i in g.indices])
        if device_output:
            return torch.cat(images)[torch.from_numpy(order).to(images[0].device)]
        return np.concatenate(images)[order]
    result = [None] * len(files)
    for g, y in zip(groups, images):
        for j, i in enumerate(g.indices):
            result[i] = y[j]
    return result


def decode_coefficients(files, device_output=False, subseq_bits=0, device=None, *, allow_restart=False, allow_progressive=False,
                        allow_grey=False, allow_sampling=False):
    """The quantised coefficients of baseline files of ONE geometry, as stored in the files: ((n, real blocks, 64) int16 in the layout
    of DESIGN.md section 4c - [Y | Cb | Cr][block row][block col][zig-zag] - and the (n, 3, 64) uint16 quantisation tables per
    component in natural order; jpeg_qf_estimation(tables[i, c].reshape(8, 8), c) names the quality they came from).
    allow_restart: as decode_batch's; the files must then share their restart interval too.  allow_progressive: as decode_batch's;
    the files must then share their scan script too (baseline files count as one script).  allow_grey: grey-scale files are read too
    - (n, blocks, 64) coefficients in raster order and (n, 1, 64) tables -, never in one call with colour files.  allow_sampling: as
    decode_batch's; the layout is the same, over the real blocks ops.jpeg_geometry names for the factors."""
    files = _as_files(files)
    headers, groups = _decode_groups(files, subseq_bits, device, _Accept(allow_restart, allow_progressive, allow_grey, allow_sampling))
    if len(groups) != 1:
        raise ValueError('decode_coefficients needs files of one geometry{}, got {}'.format(
            (' and restart interval' if allow_restart else '') + (' and scan script' if allow_progressive else ''),
            [g.geometry for g in groups]))
    _fetch_status(groups)
    coef = groups[0].coef
    return (coef if device_output else coef.cpu().numpy()), np.stack([hd.qtables for hd in headers])


def _annex_k_coding():
    """_coding's triple for Annex K's tables through the coder that takes tables: what serves the samplings that nimg_jpeg_encode does
    not.  The segments are the ones nimg_jpeg_encode writes - the same walk, the same clamps, the same codes."""
    annex_k = np.zeros((4, ops.JPEG_TABLE_BYTES), np.uint8)
    for j, t in enumerate(_DHT):
        annex_k[j, :len(t) - 1] = np.frombuffer(t, np.uint8, offset=1)

    def encode(coef, h, w, hs, vs, workspace=None, capacity=None, restart_interval=0):
        tables = torch.from_numpy(annex_k).to(coef.device).expand(coef.shape[0], 4, ops.JPEG_TABLE_BYTES).contiguous()
        return ops.jpeg_encode_tables(coef, tables, h, w, hs, vs, capacity=capacity, restart_interval=restart_interval)[:2]
    return None, encode, ops.jpeg_ecd_bound_tables


def lossless_size(h, w, hs, vs, op, crop=None, edge='perfect'):
    """(h', w', hs', vs') of the file transcode_batch(lossless=op, crop=crop, edge=edge) makes of an h x w file of the sampling factors
    (hs, vs) - ops.JPEG_GREY for a grey-scale file.  Every refusal of the transform is raised here as the same ValueError, on the host
    alone: no device is touched."""
    return ops.jpeg_lossless_geometry(h, w, hs, vs, op, crop, edge)


def _lossless_plan(headers, lossless, edge, crop):
    """What transcode_batch's lossless=, edge= and crop= ask of each file -> ([operation name per file], [(h', w', hs', vs') per file]), or
    (None, None) where nothing is asked: no operation (None or 'none' for every file) and no crop.  Host checks only; a refusal names
    the file."""
    n = len(headers)
    if lossless is None or isinstance(lossless, str):
        names = ['none' if lossless is None else lossless] * n
    else:
        names = list(lossless)
        if len(names) != n:
            raise ValueError('lossless: one operation for every file or one per file needed, got {} for {} files'.format(len(names), n))
    bad = [name for name in names if not isinstance(name, str) or name not in ops.JPEG_LOSSLESS_OPS]
    if bad:
        raise ValueError('lossless: one of {} needed, got {!r}'.format(', '.join(ops.JPEG_LOSSLESS_OPS), bad[0]))
    if edge not in ops.JPEG_LOSSLESS_EDGES:
        raise ValueError("edge: 'perfect' (refuse a partial iMCU) or 'trim' (cut it off) needed, got {!r}".format(edge))
    if crop is None and all(name == 'none' for name in names):
        return None, None
    sizes = []
    for i, (hd, name) in enumerate(zip(headers, names)):
        try:
            sizes.append(lossless_size(hd.h, hd.w, *(ops.JPEG_GREY if hd.ncomp == 1 else (hd.hs, hd.vs)), name, crop, edge))
        except ValueError as e:
            raise ValueError('file {} ({} x {}, width x height): {}'.format(i, hd.w, hd.h, e)) from None
    return names, sizes


def _transposed_tables(qt):
    """(T, 64) tables in natural order, each transposed: what a transposing operation makes of a file's quantisation tables."""
    return np.ascontiguousarray(qt.reshape(-1, 8, 8).transpose(0, 2, 1)).reshape(-1, 64)


_LOSSLESS_TRANSPOSING = ('transpose', 'transverse', 'rot90', 'rot270')


def transcode_batch(files, optimize=True, *, allow_restart=False, progressive=False, allow_progressive=False, allow_grey=False,
                    allow_sampling=False, lossless=None, edge='perfect', crop=None):
    """Baseline files written again with their coefficients and their quantisation tables untouched - a list of bytes in input order.
    The Huffman tables are the optimal ones of each image (what jpegtran -optimize does) or, with optimize=False, Annex K's.  Every
    file parse_header accepts is read; the header written is the one of encode_batch - JFIF APP0, two DQT segments where the file's Cb
    and Cr tables are equal, else three; APPn and COM segments are dropped.  Files go up in one copy, every group of equal (h, w,
    sampling) is decoded (nimg_jpeg_decode) and coded again on the device without a pixel being computed.  Damaged data raises as in
    decode_batch.  allow_restart: files with a restart interval are read too, and every file keeps its interval - DRI segment and
    markers are written again.  progressive: baseline files in, progressive files out (the lossless jpegtran -progressive); their
    tables are optimal whatever `optimize` says.  allow_progressive: progressive files of any legal scan script are read too
    (parse_header) and written as baseline files - jpegtran -optimize of a progressive file - or, with progressive, as libjpeg's simple
    progression whatever script came in.  allow_grey: grey-scale files, baseline or with allow_progressive progressive, are read too and
    written again as grey-scale baseline files (one DQT segment, the DC and AC table 0) - not with `progressive`.  allow_sampling: files
    of the samplings 4:4:0, 4:1:1, 4:1:0, 1x4 and 2x4 are read too and written again as baseline files of the same
    sampling factors - not with `progressive`, which is a ValueError for them.
    lossless: jpegtran's lossless transforms on the way - a name of ops.JPEG_LOSSLESS_OPS ('hflip', 'vflip',
    'transpose', 'transverse', 'rot90' - clockwise -, 'rot180', 'rot270', 'none') for every file, or a sequence of one name per file.
    The coefficients are permuted and re-signed on the device (ops.jpeg_lossless, one call per decode group and operation; a file whose
    operation is 'none' and that is not cropped takes none), the quantisation tables of a file are transposed by the transposing
    operations, and everything behind runs at the geometry that results: the four transposing operations swap height with width and
    the sampling factors hs with vs, so a 4:2:2 file comes out as 4:4:0 - written without allow_sampling, which reading it back needs.
    A file keeps its restart interval as the same number of MCUs.  `optimize` composes; `progressive` where the OUTPUT factors are 1x1,
    2x1 or 2x2.  crop (x, y, width, height): a region of every source file, cut before the operation (with 'none' too); x must be a
    multiple of 8 hs and y of 8 vs (8 for grey-scale) - jpegtran moves an unaligned origin down silently, here it is a ValueError that
    names the aligned value below; the blocks at a new right or bottom edge keep their contents, as jpegtran's do.  edge: a transform
    moves whole iMCUs, so hflip and rot270 need the width to be a multiple of 8 hs, vflip and rot90 the height of 8 vs, rot180 and
    transverse both; 'perfect' (jpegtran -perfect, the default) refuses a file where it is not, naming the file and the dimension,
    'trim' (jpegtran -trim) cuts the partial iMCU off first.  lossless_size names the size that results.  Every refusal is raised before
    a byte goes to the device.  None, or 'none' without a crop, is the call as it was."""
    files = _as_files(files)
    accept = _Accept(allow_restart, allow_progressive, allow_grey, allow_sampling)
    headers = [parse_header(f, *accept) for f in files]
    names, sizes = _lossless_plan(headers, lossless, edge, crop)
    _colour_only(_PROGRESSIVE_GREY, progressive and any(hd.ncomp == 1 for hd in headers))
    written = [(hd.hs, hd.vs) for hd in headers] if sizes is None else [s[2:] for s in sizes]       # the factors of the files written
    wide = sorted({f for hd, f in zip(headers, written) if hd.ncomp == 3 and ops.jpeg_is_wide(*f)})
    if progressive and wide:
        raise ValueError('progressive=True: progressive files are not written with the sampling factors {} (DESIGN.md section 8); they '
                         'are written again as baseline files'.format(', '.join('{}x{}'.format(*f) for f in wide)))
    headers, groups = _decode_groups(files, 0, None, accept, headers)
    _fetch_status(groups)
    result = [None] * len(files)
    for g in groups:
        by_op = OrderedDict()                                               # the group splits by operation: positions in the group
        for j, i in enumerate(g.indices):
            by_op.setdefault('none' if names is None else names[i], []).append(j)
        for name, at in by_op.items():
            (h, w, hs, vs), ri, coef = g.geometry, g.restart_interval, g.coef
            if len(at) != len(g.indices):
                coef = coef[torch.as_tensor(at, device=coef.device)]
            if name != 'none' or crop is not None:
                coef, h, w, hs, vs = ops.jpeg_lossless(coef, h, w, hs, vs, name, crop, edge)
            coding = _annex_k_coding() if ops.jpeg_is_wide(hs, vs) and not optimize else _coding(optimize, progressive)
            segments, tables = _device_segments(coding, coef, len(at), h, w, hs, vs, restart_interval=ri)
            for k, j in enumerate(at):                                      # a file at a time: each keeps its quantisation tables
                i = g.indices[j]
                qt = _transposed_tables(headers[i].qtables) if name in _LOSSLESS_TRANSPOSING else headers[i].qtables
                qt = qt if len(qt) == 1 else (qt[:2] if np.array_equal(qt[1], qt[2]) else qt)
                result[i], = _jpeg_files(h, w, None, (hs, vs), segments[k:k + 1], None if tables is None else tables[k:k + 1], qt, ri,
                                         progressive)
    return result


class JPEGMarkerStats(object):
    """Where the segments of a baseline JPEG file start (jpeg_helpers.py:133-250): `blocks` maps 'SOI', 'APP:<n>/<index>',
    'DQT:<id>', 'DCT' (SOF0), 'DHT:<id byte>', 'SOS', 'ECD' and 'EOI' to byte offsets ('EOI' = the file length).  `shape` is read
    from SOF0 - no decode.  Anything that cannot be parsed, progressive files included, raises IOError."""

    def __init__(self, image):
        if type(image) is str:
            with open(image, 'rb') as f:
                image = f.read()
        elif type(image) is not bytes:
            raise ValueError('Image not supported! Supported: str, bytes')
        self.blocks = OrderedDict()
        self.shape = None
        self._quantization_tables = {}
        try:
            self._scan(image)
            if 'EOI' not in self.blocks or self.shape is None:
                raise ValueError('no frame header or no end of image')
        except Exception as e:
            raise IOError('Parsing error: {}'.format(e))

    def _scan(self, data):
        order = np.argsort(zigzag(8).ravel(), kind='stable')
        pos, apps = 0, 0
        self.blocks['SOI'] = 0
        while pos < len(data):
            marker, = struct.unpack_from('>H', data, pos)
            if marker == 0xffd8:
                pos += 2
                continue
            if marker == 0xffd9:
                self.blocks['EOI'] = pos + 2
                return
            size = 2 + struct.unpack_from('>H', data, pos + 2)[0]
            body = data[pos + 4:pos + size]
            if marker == 0xffdb:
                for k in range(0, len(body), 65):
                    self.blocks['DQT:{}'.format(body[k] & 15)] = pos
                    table = np.zeros(64, np.uint8)
                    table[order] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                    self._quantization_tables[body[k] & 15] = table.reshape(8, 8)
            elif marker == 0xffc0:
                self.blocks['DCT'] = pos
                rows, cols = struct.unpack_from('>HH', body, 1)
                self.shape = (rows, cols, body[5]) if body[5] > 1 else (rows, cols)
            elif marker == 0xffc2:
                raise NotImplementedError('Progressive JPEG images not supported yet')
            elif marker == 0xffc4:
                k = 0
                while k < len(body):
                    self.blocks['DHT:{}'.format(body[k])] = pos
                    k += 17 + sum(body[k + 1:k + 17])
            elif marker == 0xffda:
                self.blocks['SOS'] = pos
                self.blocks['ECD'] = pos + size
                pos = len(data) - 2                      # a valid file ends with EOI; anything else fails on the next read
                continue
            elif 0xffe0 <= marker <= 0xffef:
                self.blocks['APP:{}/{}'.format(marker & 15, apps)] = pos
                apps += 1
            elif marker in (0xfffe, 0xffdd):
                self.blocks['RST'] = pos
            else:
                return
            pos += size

    def get_bytes(self):
        return self.blocks['EOI']

    def get_effective_bytes(self):
        return self.blocks['EOI'] - self.blocks['DHT:0']

    def get_effective_bpp(self):
        return 8 * self.get_effective_bytes() / self.shape[0] / self.shape[1]

    def get_bpp(self):
        return 8 * self.get_bytes() / self.shape[0] / self.shape[1]
