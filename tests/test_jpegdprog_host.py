"""Reading progressive JPEG files, the part that needs no GPU: parse_header on progressive files and each of
its refusals; the plain Python restatement (jpegdprog_ref) against the coefficients the files were written from and against Pillow's
pixels; the sequential core csrc/jpegdprog.h, built into tests/jpegdprog_host.cpp under the address and undefined-behaviour
sanitizers, over the Pillow files, the files of two further scan scripts, synthetic tensors and damaged streams at every subsequence
length, coefficients against the expected ones and synchronisation rounds against the restatement's."""
import importlib
import io
import struct

import numpy as np
import pytest

import jpegdprog_cases as cases
import jpegdprog_ref as dpref
import jpegprog_cases as pc
import jpegprog_ref as pref

importlib.import_module('neural-imaging_amd')
from neural_imaging_amd.compression import jpeg_helpers as jh  # noqa: E402

pytestmark = pytest.mark.skipif(cases.jpegd_cases.compiler() is None, reason='no host C++ compiler')


def _by_name(name):
    return next(f for f in cases.valid_files() if f.name == name)


# ---- parse_header -----------------------------------------------------------------------------------------------------------------
def test_parse_header_reads_every_file_and_script():
    for f in cases.golden_files() + cases.script_files():
        hd, p = jh.parse_header(f.data, allow_restart=True, allow_progressive=True), dpref.split(f.data)
        assert (hd.h, hd.w, hd.hs, hd.vs, hd.restart_interval) == (f.h, f.w, f.hs, f.vs, f.ri), f.name
        assert tuple(s[:5] for s in hd.scans) == f.script == dpref.SCRIPTS[f.name.split('|')[2]], f.name
        assert [list(s.huffman) for s in hd.scans] == p['tables'], f.name
        assert [f.data[s.ecd_offset:s.ecd_end] for s in hd.scans] == p['segments'], f.name
        assert hd.huffman == () and (hd.ecd_offset, hd.ecd_end) == (hd.scans[0].ecd_offset, len(f.data) - 2), f.name
        assert np.array_equal(hd.qtables, np.stack([p['qtables'][k] for k in p['q']])), f.name
        assert jh.jpeg_script_check([s[:5] for s in hd.scans]) == dpref.levels(f.script), f.name
        assert len(hd) == 9                            # the tuple baseline callers unpack is the one it was


def test_baseline_headers_carry_no_scans():
    import jpegd_cases
    for f in jpegd_cases.files()[:4]:
        a, b = jh.parse_header(f.data, allow_progressive=True), jh.parse_header(f.data)
        assert a[:4] + a[5:] == b[:4] + b[5:] and np.array_equal(a.qtables, b.qtables) and len(a) == 9
        assert a.scans == () == b.scans


def test_default_refuses_with_todays_words():
    data = _by_name('g_smooth_16x16_q100_444|0|std').data
    for args in ((), (True,)):
        with pytest.raises(ValueError) as e:
            jh.parse_header(data, *args)
        assert str(e.value) == 'progressive file (SOF2): only baseline sequential files (SOF0) are read'


def _segments(data):
    """[(offset, marker, whole length)] of the marker segments of a file, entropy-coded data stepped over."""
    out, i = [], 2
    while data[i + 1] != 0xd9:
        size = struct.unpack_from('>H', data, i + 2)[0]
        out.append((i, data[i + 1], 2 + size))
        i += 2 + size
        if out[-1][1] == 0xda:
            while not (data[i] == 0xff and data[i + 1] != 0 and not 0xd0 <= data[i + 1] <= 0xd7):
                i += 1
    return out


def _refused(data, match, allow_restart=True):
    with pytest.raises(ValueError, match=match):
        jh.parse_header(bytes(data), allow_restart=allow_restart, allow_progressive=True)


def test_each_refusal_names_its_reason():
    data = _by_name('mixed_37x53_q75_420_ri0|0|std').data
    segs = _segments(data)
    sos = [s for s in segs if s[1] == 0xda]
    assert len(sos) == 10

    def edited(k, ss=None, se=None, ahal=None):
        out = bytearray(data)
        end = sos[k][0] + sos[k][2]
        for at, v in ((end - 3, ss), (end - 2, se), (end - 1, ahal)):
            if v is not None:
                out[at] = v
        return out

    # an incomplete progression: the file without its last scan
    _refused(data[:sos[9][0]] + b'\xff\xd9', 'incomplete progression')
    # scripts that break the rules
    _refused(edited(1, ahal=0x12), 'illegal progressive script')          # a first scan of its coefficients with Ah = 1
    _refused(edited(5, ahal=0x10), 'illegal progressive script')          # a refinement that skips a bit (2 -> 0)
    _refused(edited(1, ss=0, se=5), 'illegal progressive script')         # DC and AC in one scan
    _refused(edited(1, ss=9, se=5), 'illegal progressive script')
    _refused(edited(2, ss=1, se=5), 'illegal progressive script|incomplete')
    _refused(edited(9, ahal=0x00), 'illegal progressive script')          # a coefficient coded first twice
    a = _by_name('mixed_37x53_q75_444_ri0|0|A').data
    sa = [s for s in _segments(a) if s[1] in (0xda, 0xc4)]
    first = next(s for s in sa if s[1] == 0xda)[0]
    y_ac = [k for k, s in enumerate(sa) if s[1] == 0xda][3]                # its DHT segment stands in front of it, the next scan's behind
    lo, hi = sa[y_ac - 1][0], sa[y_ac + 1][0]
    assert sa[y_ac - 1][1] == 0xc4 and sa[y_ac + 1][1] == 0xc4
    _refused(a[:first] + a[lo:hi] + a[first:lo] + a[hi:], 'comes before the DC first scan')       # Y's AC scan in front of its DC scan
    # the restart interval changes between scans; a DRI that repeats it is accepted
    ri = _by_name('mixed_37x53_q75_420_ri2|0|std').data
    rs = [s for s in _segments(ri) if s[1] == 0xda]
    _refused(ri[:rs[3][0]] + b'\xff\xdd\x00\x04\x00\x05' + ri[rs[3][0]:], 'restart interval changes between scans')
    _refused(data[:sos[3][0]] + b'\xff\xdd\x00\x04\x00\x05' + data[sos[3][0]:], 'restart interval changes between scans')
    jh.parse_header(ri[:rs[3][0]] + b'\xff\xdd\x00\x04\x00\x02' + ri[rs[3][0]:], True, True)
    _refused(ri, 'restart interval', allow_restart=False)
    # DNL, other markers between scans, COM and APPn accepted
    _refused(data[:sos[1][0]] + b'\xff\xdc\x00\x04\x00\x25' + data[sos[1][0]:], 'DNL')
    dqt = next(s for s in segs if s[1] == 0xdb)
    _refused(data[:sos[1][0]] + data[dqt[0]:dqt[0] + dqt[2]] + data[sos[1][0]:], 'unsupported marker FFDB between the scans')
    ok = data[:sos[1][0]] + b'\xff\xfe\x00\x04hi' + b'\xff\xe1\x00\x03x' + data[sos[1][0]:]
    assert [s[:5] for s in jh.parse_header(ok, True, True).scans] == list(dpref.STANDARD)
    # arithmetic coding, 12-bit samples, grey-scale
    sof = next(s for s in segs if s[1] == 0xc2)
    arith = bytearray(data)
    arith[sof[0] + 1] = 0xca
    _refused(arith, 'arithmetic-coded progressive file')
    deep = bytearray(data)
    deep[sof[0] + 4] = 12
    _refused(deep, '12-bit samples')
    # a missing table: the DHT segment in front of the first AC scan taken out
    dht = [s for s in segs if s[1] == 0xc4 and s[0] < sos[1][0]][-1]
    assert dht[0] > sos[0][0]
    _refused(data[:dht[0]] + data[dht[0] + dht[2]:], 'missing Huffman table: AC table 0 of component 0 in scan 1')


def test_every_truncation_is_a_value_error():
    data = _by_name('g_smooth_8x8_q50_444|0|std').data
    first = jh.parse_header(data, allow_progressive=True).scans[0].ecd_offset
    for cut in range(first - 12, len(data)):
        with pytest.raises(ValueError):
            jh.parse_header(data[:cut], allow_progressive=True)


def test_more_than_64_scans_are_refused():
    case = pc.by_name('g_smooth_8x8_q50_444')
    coefs = pc.reference(case).coefs[0]
    prefix = pref.prefix_of(pc.baseline_header(case))
    head = [((c,), 0, 0, 0, 0) for c in range(3)] + [((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]
    script64 = head + [((0,), k, k, 0, 0) for k in range(1, 59)] + [((0,), 59, 63, 0, 0)]
    script65 = head + [((0,), k, k, 0, 0) for k in range(1, 60)] + [((0,), 60, 63, 0, 0)]
    assert (len(script64), len(script65)) == (64, 65) and dpref.legal(script64)
    hd = jh.parse_header(dpref.encode(coefs, 8, 8, 1, 1, prefix, script64), allow_progressive=True)
    assert len(hd.scans) == 64
    with pytest.raises(ValueError, match='more than 64 scans'):
        jh.parse_header(dpref.encode(coefs, 8, 8, 1, 1, prefix, script65), allow_progressive=True)
    f = cases._file('64scans', dpref.encode(coefs, 8, 8, 1, 1, prefix, script64), pc.reference(case).flat[0])
    host, done = cases.host_results([f], settings=(32, 0))
    assert done.returncode == 0, done.stderr.decode()
    assert host[0].levels == [1] * 64 and all(np.array_equal(host[0].coef[v], f.expected) and host[0].status[v] == 0 for v in (32, 0))


# ---- the writers of the test files ---------------------------------------------------------------------------------------------
def test_script_writer_reproduces_the_stored_and_pillows_files():
    stored = cases.stored()[0]
    for script in ('A', 'B'):
        for name in cases.SCRIPT_CASES:
            assert cases.script_file(name, script) == stored['{}|{}'.format(name, script)], (name, script)
    for name in ('mixed_37x53_q75_420_ri3', 'mixed_40x56_three_422', 'g_noise_13x21_q5_420'):           # libjpeg's script: Pillow's bytes
        case = pc.by_name(name)
        hs, vs = pref.ref.SUBSAMPLING[case.subsampling]
        data = dpref.encode(pc.reference(case).coefs[0], case.h, case.w, hs, vs, pref.prefix_of(pc.baseline_header(case)), dpref.STANDARD,
                            case.ri)
        assert data == pc.golden()[name][0], name


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_levels():
    # every coefficient passes one first scan and one refinement per bit plane below its first Al, so the levels of a script are
    # 1 + the highest first Al of a band that is refined: libjpeg's script 3 (scans 1-5, 6-9, 10), A 1 (no refinement), B 3
    assert dpref.levels(dpref.STANDARD) == [1, 1, 1, 1, 1, 2, 2, 2, 2, 3]
    assert dpref.levels(dpref.SCRIPT_A) == [1] * 6
    assert dpref.levels(dpref.SCRIPT_B) == [1] * 5 + [2] * 4 + [3] * 5
    assert all(dpref.legal(s) for s in dpref.SCRIPTS.values())


@pytest.fixture(scope='module')
def restated():
    """The restatement over every quick valid file at one subsequence per interval: {name: (coef, status, rounds)}."""
    out = {}
    for f in cases.valid_files(slow=False):
        tables = [[(bytes(t[:16]), bytes(t[16:16 + int(t[:16].sum())])) for t in tt[:len(sc[0])]] for tt, sc in zip(f.tables, f.script)]
        out[f.name] = dpref.decode_scans(f.h, f.w, f.hs, f.vs, f.ri, f.script, tables, f.segments, 0), tables
    return out


def test_restatement_returns_the_coefficients(restated):
    assert len(restated) == 71 + 30 + 5
    for f in cases.valid_files(slow=False):
        (coef, status, rounds), _ = restated[f.name]
        assert status == 0 and rounds == [0] * len(f.script), f.name
        assert np.array_equal(coef, f.expected), f.name


def test_restatement_pixels_are_pillows():
    Image = pytest.importorskip('PIL.Image')
    crcs = cases.stored()[1]
    for f in cases.golden_files() + cases.script_files():
        if f.slow or f.h * f.w > 64 * 64:
            continue
        rgb = dpref.decode_u8(f.data)
        assert np.array_equal(rgb, np.asarray(Image.open(io.BytesIO(f.data)).convert('RGB'))), f.name
        assert cases.crc(rgb) == crcs[f.name], f.name


def test_stored_checksums_are_pillows():
    Image = pytest.importorskip('PIL.Image')
    crcs = cases.stored()[1]
    files = cases.golden_files() + cases.script_files()
    assert len(crcs) == len(files) == 72 + 30
    for f in files:
        if not f.slow:
            assert cases.crc(np.asarray(Image.open(io.BytesIO(f.data)).convert('RGB'))) == crcs[f.name], f.name


# ---- the host program ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hosted():
    files = cases.valid_files(slow=True)
    host, done = cases.host_results(files)
    assert done.returncode == 0, done.stderr.decode()[-4000:]
    return files, host


def test_host_program_decodes_every_valid_file_at_every_setting(hosted):
    files, host = hosted
    assert len(files) == 72 + 30 + 5
    for f, h in zip(files, host):
        assert h.legal and h.levels == dpref.levels(f.script), f.name
        for v in cases.SETTINGS:
            assert h.status[v] == 0, (f.name, v, h.status[v])
            assert np.array_equal(h.coef[v], f.expected), (f.name, v)
        assert h.rounds[0] == [0] * len(f.script), f.name
        assert all(r == 0 for v in cases.SETTINGS for r, sc in zip(h.rounds[v], f.script) if sc[3]), f.name
    # the short settings do synchronise, and a first scan of more than 256 subsequences is among them (the chunk seam)
    big = next(h for f, h in zip(files, host) if f.name == 'mixed_128x192_q75_420_ri5|0|std')
    assert max(max(h.rounds[32]) for h in host) >= 2 and max(big.rounds[32]) >= 1


@pytest.mark.parametrize('setting', [32, 64, 256, 2048])
def test_host_rounds_are_the_restatements(hosted, restated, setting):
    files, host = hosted
    for f, h in zip(files, host):
        if f.slow or (setting in (64, 256) and f.h * f.w > 64 * 64):
            continue                                   # the restatement is plain Python: the large images at the two ends only
        coef, status, rounds = dpref.decode_scans(f.h, f.w, f.hs, f.vs, f.ri, f.script, restated[f.name][1], f.segments, setting)
        assert status == 0 and np.array_equal(coef, f.expected), (f.name, setting)
        assert rounds == h.rounds[setting], (f.name, setting)


def test_host_program_ends_damaged_streams_with_a_status():
    files = cases.damaged_files()
    assert len(files) >= 300
    host, done = cases.host_results(files)
    assert done.returncode == 0, done.stderr.decode()[-4000:]            # clean under both sanitizers
    kinds = {}
    for f, h in zip(files, host):
        tag = f.name.split('|')[3].rstrip('0123456789.')
        for v in cases.SETTINGS:
            kinds.setdefault(tag, []).append(h.status[v])
        if tag in ('cut', 'allff', 'empty', 'marker', 'longrun'):
            assert all(h.status[v] != 0 for v in cases.SETTINGS), f.name
        if tag == 'longrun':
            assert all(h.status[v] & dpref.ST_RUN for v in cases.SETTINGS), f.name
        if tag == 'marker':
            assert all(h.status[v] & dpref.ST_RESTART for v in cases.SETTINGS), f.name
    assert set(kinds) == {'cut', 'flip', 'random', 'allff', 'empty', 'marker', 'longrun'}
    assert any(kinds['flip']) and any(kinds['random'])


def test_host_program_refuses_illegal_scripts():
    f = _by_name('g_smooth_8x8_q50_444|0|std')
    std = list(dpref.STANDARD)
    illegal = [std[:9],                                                            # incomplete
               std[1:],                                                            # AC before DC
               [std[0], ((0,), 1, 5, 1, 2)] + std[2:],                             # a first scan with Ah
               std[:5] + [((0,), 1, 63, 2, 0)] + std[6:],                          # a refinement that skips a bit
               [((0, 1), 0, 0, 0, 1)] + std[1:],                                   # two components
               [std[0], ((0, 1, 2), 1, 5, 0, 2)] + std[2:],                        # an interleaved AC scan
               [std[0], ((0,), 0, 5, 0, 2)] + std[2:],                             # DC and AC in one scan
               std + [std[9]],                                                     # a bit refined twice
               []]
    for script in illegal:
        assert not dpref.legal(script)
    probes = [f._replace(script=tuple(s), tables=[f.tables[0]] * len(s), segments=[b''] * len(s)) for s in illegal]
    host, done = cases.host_results(probes + [f], settings=(0,))
    assert done.returncode == 0, done.stderr.decode()
    assert [h.legal for h in host] == [False] * len(illegal) + [True]
