"""The host structure of the JPEG reader, the part that needs no GPU: what parse_header does with fill bytes
- refused in a baseline file, stepped over and counted into the scan's span in a progressive one -, which refusal wins where a file has
two defects, and the entry point ops._jpeg_entry names for every operation at a standard sampling, for grey-scale and for a wide
sampling, against a list written out here."""
import importlib
import io
import itertools
import struct

import pytest

importlib.import_module('neural-imaging_amd')
from neural_imaging_amd import _lib, ops  # noqa: E402
from neural_imaging_amd.compression import jpeg_helpers as jh  # noqa: E402

Image = pytest.importorskip('PIL.Image')
ALL = dict(allow_restart=True, allow_progressive=True, allow_grey=True, allow_sampling=True)


def _file(h, w, progressive=False):
    """Pillow's 4:4:4 quality-80 file of a fixed h x w image: baseline with the Annex K tables, or progressive."""
    import jpeg_cases
    out = io.BytesIO()
    Image.fromarray(jpeg_cases._image('mixed', h, w, 7)).save(out, 'JPEG', quality=80, subsampling=0, progressive=progressive)
    return out.getvalue()


BASELINE, PROGRESSIVE = _file(16, 24), _file(24, 40, progressive=True)


def _segments(data, start=2):
    """[(offset, marker, body offset)] of the marker segments from `start` up to and including the next SOS."""
    out, i = [], start
    while True:
        out.append((i, data[i + 1], i + 4))
        if data[i + 1] == 0xda:
            return out
        i += 2 + struct.unpack_from('>H', data, i + 2)[0]


def _patched(data, edits):
    out = bytearray(data)
    for at, value in edits.items():
        out[at] = value
    return bytes(out)


def _inserted(data, pieces):
    """`pieces` {offset: bytes} put into the file, each in front of the byte that stands at its offset."""
    for at in sorted(pieces, reverse=True):
        data = data[:at] + pieces[at] + data[at:]
    return data


def _spans(hd):
    return [(s.ecd_offset, s.ecd_end) for s in hd.scans]


def _message(data, **allow):
    with pytest.raises(ValueError) as e:
        jh.parse_header(data, **allow)
    return str(e.value)


# ---- fill bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('allow', list(itertools.product((False, True), repeat=4)))
def test_a_baseline_file_with_a_fill_byte_before_eoi_is_refused(allow):
    hd = jh.parse_header(BASELINE, *allow)
    assert BASELINE[hd.ecd_end:] == b'\xff\xd9'
    filled = BASELINE[:-2] + b'\xff' + BASELINE[-2:]
    with pytest.raises(ValueError) as e:
        jh.parse_header(filled, *allow)                              # positionally, as _decode_groups calls it
    assert str(e.value) == 'unexpected marker FFFF in the entropy-coded segment'


def test_a_progressive_file_takes_a_fill_byte_behind_scan_0_into_its_span():
    hd = jh.parse_header(PROGRESSIVE, **ALL)
    spans = _spans(hd)
    assert len(spans) == 10 and PROGRESSIVE[spans[0][1]] == 0xff and PROGRESSIVE[spans[0][1] + 1] == 0xc4
    got = jh.parse_header(_inserted(PROGRESSIVE, {spans[0][1]: b'\xff'}), **ALL)
    assert _spans(got) == [(spans[0][0], spans[0][1] + 1)] + [(lo + 1, hi + 1) for lo, hi in spans[1:]]
    assert (got.ecd_offset, got.ecd_end) == (hd.ecd_offset, hd.ecd_end + 1)
    assert [s[:6] for s in got.scans] == [s[:6] for s in hd.scans]
    assert _spans(jh.parse_header(_inserted(PROGRESSIVE, {spans[0][1]: b'\xff'}), False, True)) == _spans(got)


def test_a_progressive_file_takes_a_fill_byte_before_eoi_into_the_last_span():
    hd = jh.parse_header(PROGRESSIVE, **ALL)
    spans = _spans(hd)
    assert hd.ecd_end == spans[-1][1] == len(PROGRESSIVE) - 2
    got = jh.parse_header(_inserted(PROGRESSIVE, {hd.ecd_end: b'\xff'}), **ALL)
    assert _spans(got) == spans[:-1] + [(spans[-1][0], spans[-1][1] + 1)]
    assert (got.ecd_offset, got.ecd_end) == (hd.ecd_offset, hd.ecd_end + 1)


def test_a_progressive_file_steps_over_a_fill_byte_between_dht_and_sos():
    hd = jh.parse_header(PROGRESSIVE, **ALL)
    spans = _spans(hd)
    (dht, marker, _), (sos, last, _) = _segments(PROGRESSIVE, spans[0][1])
    assert (marker, last) == (0xc4, 0xda) and dht == spans[0][1]
    got = jh.parse_header(_inserted(PROGRESSIVE, {sos: b'\xff'}), **ALL)
    assert _spans(got) == spans[:1] + [(lo + 1, hi + 1) for lo, hi in spans[1:]]           # no span holds it
    assert [s[:6] for s in got.scans] == [s[:6] for s in hd.scans]


# ---- the order of refusals ---------------------------------------------------------------------------------------------------------
def _baseline_marks():
    """Offsets in BASELINE: the id byte of the DQT segment of table 0, that of the DHT segment of AC table 0, the SOS body."""
    segs = _segments(BASELINE)
    dqt = next(body for _, m, body in segs if m == 0xdb and BASELINE[body] == 0)
    dht = next(body for _, m, body in segs if m == 0xc4 and BASELINE[body] == 0x10)
    sos = segs[-1][2]
    assert BASELINE[sos:sos + 10] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return dqt, dht, sos


def test_baseline_a_missing_huffman_table_is_named_before_the_components_quantisation_table():
    dqt, dht, _ = _baseline_marks()
    assert _message(_patched(BASELINE, {dqt: 3})) == 'missing quantisation table 0 of component 0'
    assert _message(_patched(BASELINE, {dht: 0x12})) == 'missing Huffman table: AC table 0 of component 0'
    for allow in ({}, ALL):
        assert _message(_patched(BASELINE, {dqt: 3, dht: 0x12}), **allow) == 'missing Huffman table: AC table 0 of component 0'


def test_baseline_the_shape_of_the_scan_is_checked_before_its_tables():
    dqt, dht, sos = _baseline_marks()
    for allow in ({}, ALL):
        assert _message(_patched(BASELINE, {sos + 8: 62, dqt: 3}), **allow) == 'not a baseline scan: Ss=0 Se=62 Ah/Al=00 (0, 63, 00 needed)'
        assert _message(_patched(BASELINE, {sos + 8: 62, dht: 0x12}), **allow) == 'not a baseline scan: Ss=0 Se=62 Ah/Al=00 (0, 63, 00 needed)'
        # two components listed in a segment that is as long as one of three
        assert _message(_patched(BASELINE, {sos: 2}), **allow) == 'malformed SOS segment'


def _scan_marks(hd, k):
    """Offsets in PROGRESSIVE of scan k's last selector, Ss, Se and Ah/Al bytes: the four in front of its entropy-coded segment."""
    at = hd.scans[k].ecd_offset
    return at - 4, at - 3, at - 2, at - 1


def test_progressive_the_script_is_checked_before_the_quantisation_tables():
    hd = jh.parse_header(PROGRESSIVE, **ALL)
    dqt = next(body for _, m, body in _segments(PROGRESSIVE) if m == 0xdb and PROGRESSIVE[body] == 0)
    assert _message(_patched(PROGRESSIVE, {dqt: 3}), **ALL) == 'missing quantisation table 0 of component 0'
    _, _, se, _ = _scan_marks(hd, 0)
    assert hd.scans[0][:5] == ((0, 1, 2), 0, 0, 0, 1)
    want = 'illegal progressive script: scan 0 (components [0, 1, 2] Ss=0 Se=5 Ah=0 Al=1) mixes DC and AC coefficients'
    assert _message(_patched(PROGRESSIVE, {se: 5}), **ALL) == want
    assert _message(_patched(PROGRESSIVE, {se: 5, dqt: 3}), **ALL) == want


def test_progressive_a_missing_table_of_an_earlier_scan_is_named_before_the_script():
    hd = jh.parse_header(PROGRESSIVE, **ALL)
    assert hd.scans[3][:5] == ((1,), 1, 63, 0, 1) and hd.scans[5][:5] == ((0,), 1, 63, 2, 1)
    sel, _, _, _ = _scan_marks(hd, 3)
    _, _, _, ahal = _scan_marks(hd, 5)
    assert PROGRESSIVE[sel] == 0x01 and PROGRESSIVE[ahal] == 0x21
    script = ('illegal progressive script: scan 5 (components [0] Ss=1 Se=63 Ah=3 Al=1) - a first scan has Ah = 0 and is the first of its '
              'coefficients, a refinement has Ah = the Al before it and Al = Ah - 1')
    assert _message(_patched(PROGRESSIVE, {ahal: 0x31}), **ALL) == script
    table = 'missing Huffman table: AC table 3 of component 1 in scan 3'
    assert _message(_patched(PROGRESSIVE, {sel: 0x03}), **ALL) == table
    assert _message(_patched(PROGRESSIVE, {sel: 0x03, ahal: 0x31}), **ALL) == table


def test_progressive_of_a_changed_dri_and_a_dnl_the_first_in_the_file_is_named():
    hd = jh.parse_header(PROGRESSIVE, **ALL)
    first, second = hd.scans[0].ecd_end, hd.scans[1].ecd_end
    dri, dnl = bytes.fromhex('ffdd00040005'), bytes.fromhex('ffdc00040018')
    changed = 'the restart interval changes between scans (0 then 5): not read'
    assert _message(_inserted(PROGRESSIVE, {first: dri}), **ALL) == changed
    assert _message(_inserted(PROGRESSIVE, {second: dnl}), **ALL) == 'DNL marker behind scan 1: not read'
    assert _message(_inserted(PROGRESSIVE, {first: dri, second: dnl}), **ALL) == changed
    assert _message(_inserted(PROGRESSIVE, {first: dnl, second: dri}), **ALL) == 'DNL marker behind scan 0: not read'


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
# (operation, the further arguments ops.py passes with it) for every call of _jpeg_entry in ops.py, and what it returned for the
# factors (2, 2), ops.JPEG_GREY and (4, 1) before the table was written: None = a ValueError (no wide-sampling form).  Left out: the three
# progressive writer operations with ops.JPEG_GREY, which no caller passes (_jpeg_colour_only refuses before) and for which the string
# replacement gave names of entry points that do not exist.
ENTRIES = [
    (('nimg_jpeg_encode_restart_workspace_bytes',), 'nimg_jpeg_grey_workspace_bytes', (), None, None),
    (('nimg_jpeg_workspace_bytes', 0), 'nimg_jpeg_grey_workspace_bytes', (0,), 'nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes', (4, 1, 1)),
    (('nimg_jpeg_transform',), 'nimg_jpeg_grey_transform', (), None, None),
    (('nimg_jpeg_transform_tables',), 'nimg_jpeg_grey_transform_tables', (), None, None),
    (('nimg_jpeg_encode_restart',), 'nimg_jpeg_grey_encode', (), None, None),
    (('nimg_jpeg_encode_tables_restart',), 'nimg_jpeg_grey_encode_tables', (), 'nimg_jpeg_sampling_encode_tables', (4, 1)),
    (('nimg_jpeg_encode_tables_restart_workspace_bytes',), 'nimg_jpeg_grey_encode_tables_workspace_bytes', (),
     'nimg_jpeg_sampling_encode_tables_workspace_bytes', (4, 1)),
    (('nimg_jpeg_histogram_restart',), 'nimg_jpeg_grey_histogram', (), 'nimg_jpeg_sampling_histogram', (4, 1)),
    (('nimg_jpeg_decode_restart',), 'nimg_jpeg_grey_decode', (), 'nimg_jpeg_sampling_decode', (4, 1)),
    (('nimg_jpeg_decode_restart_workspace_bytes',), 'nimg_jpeg_grey_decode_workspace_bytes', (), 'nimg_jpeg_sampling_decode_workspace_bytes', (4, 1)),
    (('nimg_jpeg_decode_progressive',), 'nimg_jpeg_grey_decode_progressive', (), 'nimg_jpeg_sampling_decode_progressive', (4, 1)),
    (('nimg_jpeg_decode_progressive_workspace_bytes',), 'nimg_jpeg_grey_decode_progressive_workspace_bytes', (),
     'nimg_jpeg_sampling_decode_progressive_workspace_bytes', (4, 1)),
    (('nimg_jpeg_reconstruct_tables',), 'nimg_jpeg_grey_reconstruct_tables', (), 'nimg_jpeg_sampling_reconstruct_tables', (4, 1)),
    (('nimg_jpeg_reconstruct_scaled',), 'nimg_jpeg_reconstruct_scaled_grey', (), 'nimg_jpeg_sampling_reconstruct_scaled', (4, 1)),
    (('nimg_jpeg_reconstruct_scaled_workspace_bytes',), 'nimg_jpeg_reconstruct_scaled_grey_workspace_bytes', (),
     'nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes', (4, 1)),
    (('nimg_jpeg_encode_progressive',), None, None, None, None),
    (('nimg_jpeg_progressive_workspace_bytes',), None, None, None, None),
    (('nimg_jpeg_progressive_histogram',), None, None, None, None),
]


def test_every_operation_names_the_entry_point_it_named():
    assert ops.JPEG_GREY == (0, 0) and ops.jpeg_is_wide(4, 1)
    for (name, *more), grey, grey_args, wide, wide_args in ENTRIES:
        assert ops._jpeg_entry(name, 2, 2, *more) == (name, (2, 2)), name
        if grey is not None:
            assert ops._jpeg_entry(name, *ops.JPEG_GREY, *more) == (grey, grey_args), name
        if wide is not None:
            assert ops._jpeg_entry(name, 4, 1, *more) == (wide, wide_args), name
            continue
        with pytest.raises(ValueError) as e:
            ops._jpeg_entry(name, 4, 1, *more)
        assert str(e.value) == ('{}: the sampling factors 4x1 are only read from files and written again with their coefficients (decode, '
                                'reconstruct, histogram, encode_tables)'.format(name.replace('nimg_', ''))), name


def test_every_entry_point_named_is_declared_in_the_header():
    named = {name for (name, *_), _, _, _, _ in ENTRIES}
    for (name, *more), grey, _, wide, _ in ENTRIES:
        named |= {ops._jpeg_entry(name, *f, *more)[0] for f, there in ((ops.JPEG_GREY, grey), ((4, 1), wide)) if there}
    assert len(named) == 18 + 14 + 10
    assert not sorted(named - set(_lib.PROTOTYPES))
