"""The host side of the rate-distortion feature (no GPU): the ABI of the per-item JPEG and MS-SSIM entry points, the cached tables
of compression.ratedistortion and the argument checks that come before any device work."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import ratedist_cases as cases
from neural_imaging_amd import _lib
from neural_imaging_amd.compression import codec, jpeg_helpers as jh, ratedistortion as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nimg_jpeg_transform_items', 'nimg_jpeg_reconstruct_items', 'nimg_msssim_workspace_bytes', 'nimg_msssim')


# ---- 8. binding and header ---------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_version_8():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nimg.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(nimg_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    # the number of arguments the binding passes is the number the header declares
    for name in NEW:
        args = re.search(r'\b{}\s*\(([^)]*)\)'.format(name), header).group(1)
        assert len(_lib.PROTOTYPES[name][1]) == len([a for a in args.split(',') if a.strip() and a.strip() != 'void']), name
    assert int(re.search(r'#define\s+NIMG_ABI_VERSION\s+(\d+)', header).group(1)) == 8 == _lib.ABI_VERSION
    assert _lib.load().nimg_abi_version() == 8


def test_workspace_sizes_need_no_device():
    lib = _lib.load()
    assert lib.nimg_msssim_workspace_bytes(2, 176, 192, 3) > 2 * 2 * 88 * 96 * 3 * 4
    for n, h, w, c in ((1, 168, 176, 3), (1, 176, 160, 3), (1, 180, 176, 3), (0, 176, 176, 3), (1, 176, 176, 0)):
        assert lib.nimg_msssim_workspace_bytes(n, h, w, c) == 0, (n, h, w, c)          # the size rule: multiples of 16, at least 176
    # an item call sizes its workspace by the number of items
    assert lib.nimg_jpeg_workspace_bytes(12, 64, 72, 2, 1) > lib.nimg_jpeg_workspace_bytes(4, 64, 72, 2, 1) > 0


# ---- 9. cached tables ----------------------------------------------------------------------------------------------------------
class Reached(Exception):
    pass


def _raise(*a, **k):
    raise Reached()


JPEG_CSV = ('image_id,filename,codec,quality,ssim,psnr,msssim,msssim_db,bytes,bpp\n'
            '0,a.png,jpeg,95,0.98,40.5,0.99,20.0,1234,0.75\n'
            '0,a.png,jpeg,90,0.97,38.25,0.985,18.5,1000,0.5\n')
DCN_CSV = ('image_id,filename,model_dir,codec,ssim,psnr,msssim,msssim_db,entropy,bytes,bpp,layers,quantization,entropy_reg,codebook,'
           'latent,latent_shape,n_features\n'
           '0,a.png,run0/,TwitterDCN-4C/x,0.9,30.5,0.95,13.0,2.5,321,0.125,,soft-codebook-5bpf,250.0,soft-codebook,1936,22x22x4,4\n')


def test_cached_tables_are_returned_without_the_device(tmp_path, monkeypatch):
    images, models = tmp_path / 'images', tmp_path / 'models'
    (models / 'run0' / 'twitterdcn').mkdir(parents=True)
    images.mkdir()
    with open(str(models / 'run0' / 'twitterdcn' / 'progress.json'), 'w') as f:
        json.dump({'codec': {'model': 'TwitterDCN', 'args': {}}}, f)
    cases.write_pngs(images, 32, 48)
    (images / 'jpeg.csv').write_text(JPEG_CSV)
    (images / 'dcn-models.csv').write_text(DCN_CSV)
    for mod, name in ((jh, 'rate_distortion'), (jh, 'compress_batch'), (codec, 'restore'), (codec, 'compress_n_stats')):
        monkeypatch.setattr(mod, name, _raise)
    df = rd.get_jpeg_df(str(images))
    assert list(df.columns) == rd.JPEG_COLUMNS and df['quality'].tolist() == [95, 90] and df['bytes'].tolist() == [1234, 1000]
    assert df['bpp'].tolist() == [0.75, 0.5] and df['filename'].tolist() == ['a.png', 'a.png']
    dd = rd.get_dcn_df(str(images), str(models) + os.sep)                     # (a trailing separator names the same file)
    assert list(dd.columns) == rd.DCN_COLUMNS and dd['bytes'].tolist() == [321] and dd['latent_shape'].tolist() == ['22x22x4']
    assert rd.get_dcn_df(str(images), str(models))['n_features'].tolist() == [4]
    with pytest.raises(Reached):
        rd.get_jpeg_df(str(images), force_calc=True)
    with pytest.raises(Reached):
        rd.get_dcn_df(str(images), str(models), force_calc=True)
    assert (images / 'jpeg.csv').read_text() == JPEG_CSV and (images / 'dcn-models.csv').read_text() == DCN_CSV


def test_columns_are_the_reference_tables():
    assert rd.JPEG_COLUMNS == ['image_id', 'filename', 'codec', 'quality', 'ssim', 'psnr', 'msssim', 'msssim_db', 'bytes', 'bpp']
    assert rd.DCN_COLUMNS == ['image_id', 'filename', 'model_dir', 'codec', 'ssim', 'psnr', 'msssim', 'msssim_db', 'entropy', 'bytes', 'bpp',
                              'layers', 'quantization', 'entropy_reg', 'codebook', 'latent', 'latent_shape', 'n_features']


# ---- 10. argument checks before any device work --------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_device(monkeypatch):
    monkeypatch.setattr(jh, '_device_batch', _raise)                          # the upload: nothing may get this far
    x = np.zeros((2, 16, 16, 3), np.float32)
    for bad in ([0], [101], [50, 0, 75], [], [50.5], np.array([[95, 300]])):
        with pytest.raises(ValueError, match='Invalid JPEG qualit'):
            jh.rate_distortion(x, bad)
    from neural_imaging_amd import ops
    for bad in ([50.5, 75], [0, 75], [50, 101], ['a', 'b']):
        with pytest.raises(ValueError, match='Invalid JPEG quality'):
            ops.jpeg_item_qualities(bad, 2, None)
    with pytest.raises(ValueError, match='2 values needed'):
        ops.jpeg_item_qualities([50], 2, None)
    with pytest.raises(ValueError, match='sub-sampling'):
        jh.rate_distortion(x, [50], subsampling='4:1:1')
    with pytest.raises(ValueError, match='target'):
        jh.match_quality_batch(x, [0.9, 0.9, 0.9])
    with pytest.raises(ValueError, match='target'):
        jh.match_quality_batch(x, np.full((2, 1), 0.9))
    for match in ('psnr', 'msssim', None):
        with pytest.raises(ValueError, match='Invalid argument: match'):
            jh.match_quality_batch(x, 0.9, match)
    with pytest.raises(ValueError, match='batch'):
        jh.match_quality_batch(x[0], 0.9)
    with pytest.raises(Reached):
        jh.match_quality_batch(x, [0.9, 0.8])                                 # well-formed: goes on to the device
    with pytest.raises(Reached):
        jh.rate_distortion(x, np.arange(95, 5, -5))


def test_match_targets_are_bracketed_by_the_restatement():
    """The targets of the GPU test of match_quality_batch come from the restatement; its end points bracket them (no GPU)."""
    import jpeg_ref as ref
    x = cases.match_images()
    u8 = ref.to_bytes(x)
    assert np.array_equal(u8.astype(np.float32) / np.float32(255), x)
    sizes = np.array([[len(ref.encode(img, q)) for q in (1, 15, 40, 65, 88, 95)] for img in u8])
    assert (np.diff(sizes, axis=1) > 0).all()
