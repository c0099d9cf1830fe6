"""
Rate-distortion tables - the reference's compression/ratedistortion.py: get_jpeg_df (:23-84) and get_dcn_df (:238-312) with their
arguments, column names and order, row order (image-major; JPEG qualities 95, 90, ... 10), CSV names (jpeg.csv, dcn-<last component
of the model directory>.csv) and caching rule (an existing CSV is read and returned unless force_calc; nothing touches the device
then).  A cached CSV is parsed with float_precision='round_trip', so it holds the numbers that were computed.  write_files leaves
the same PNGs (<image stem>/jpeg_q095.png ..., <image stem>/<model code>.png), written through PIL.

  get_jpeg_df   one jpeg_helpers.rate_distortion call over the directory's images: the whole sweep is coded as qualities x images
                items of the per-item JPEG kernels instead of one compress_batch call per image and quality
  get_dcn_df    every model under model_directory with a progress.json, restored at the images' size; per-image numbers from
                codec.compress_n_stats over batches of DCN_BATCH images

The msssim / msssim_db columns are helpers.metrics.msssim = tf.image.ssim_multiscale(a, b, 1.0); the reference fills them from
sewar.full_ref.msssim, and the two are not pinned against each other.  Images too small for it get nan.

Out of scope: get_jpeg2k_df and get_bpg_df (they shell out to glymur and bpgenc) and the plotting functions (seaborn) - none of
the three packages is available to this project; load_data reads the CSVs written here as they are.
"""
import json
import os
from pathlib import Path

import numpy as np

from . import codec, jpeg_helpers
from ..helpers import loading, metrics

JPEG_COLUMNS = ['image_id', 'filename', 'codec', 'quality', 'ssim', 'psnr', 'msssim', 'msssim_db', 'bytes', 'bpp']
DCN_COLUMNS = ['image_id', 'filename', 'model_dir', 'codec', 'ssim', 'psnr', 'msssim', 'msssim_db', 'entropy', 'bytes', 'bpp', 'layers',
               'quantization', 'entropy_reg', 'codebook', 'latent', 'latent_shape', 'n_features']
DCN_BATCH = 8                     # images per compress_n_stats call


def _load(directory):
    files, _ = loading.discover_images(directory, n_images=-1, v_images=0)
    batch_x = loading.load_images(files, directory, load='y')
    return files, batch_x['y'].astype(np.float32) / (2 ** 8 - 1)


def _write_png(directory, filename, name, image):
    from PIL import Image
    image_dir = os.path.join(directory, os.path.splitext(filename)[0])
    os.makedirs(image_dir, exist_ok=True)
    Image.fromarray((255 * image).astype(np.uint8)).save(os.path.join(image_dir, name))


def get_jpeg_df(directory, write_files=False, effective_bytes=True, force_calc=False, optimize=False):
    """The rate-distortion curve of JPEG over the images of `directory` as a pandas DataFrame, saved as <directory>/jpeg.csv; if that
    file exists it is read and returned instead.  With `optimize` the byte counts are those of files with optimised Huffman tables and
    the file is <directory>/jpeg-optimized.csv, so that a cached jpeg.csv is never taken for it."""
    import pandas as pd
    df_path = os.path.join(directory, 'jpeg-optimized.csv' if optimize else 'jpeg.csv')
    if os.path.isfile(df_path) and not force_calc:
        return pd.read_csv(df_path, index_col=False, float_precision='round_trip')
    files, batch_x = _load(directory)
    quality_levels = np.arange(95, 5, -5)
    rd = jpeg_helpers.rate_distortion(batch_x, quality_levels, effective=effective_bytes, want_images=write_files, optimize=optimize)
    if write_files:
        rd, decoded = rd
        decoded = decoded.cpu().numpy()
    rows = []
    for image_id, filename in enumerate(files):
        for qi, q in enumerate(quality_levels):
            if write_files:
                _write_png(directory, filename, 'jpeg_q{:03d}.png'.format(q), decoded[qi, image_id])
            rows.append({'image_id': image_id, 'filename': filename, 'codec': 'jpeg', 'quality': int(q),
                         'ssim': rd['ssim'][qi, image_id], 'psnr': rd['psnr'][qi, image_id], 'msssim': rd['msssim'][qi, image_id],
                         'msssim_db': rd['msssim_db'][qi, image_id], 'bytes': int(rd['bytes'][qi, image_id]),
                         'bpp': rd['bpp'][qi, image_id]})
    df = pd.DataFrame(rows, columns=JPEG_COLUMNS)
    df.to_csv(df_path, index=False)
    return df


def _restore_dcn(model_dir, patch_size):
    """The model of a training directory.  codec.restore reads the reference's training log ('codec': {'model', 'args'});
    training.compression.train_dcn of this project writes 'args' at the top level - both are restored."""
    with open(os.path.join(model_dir, 'progress.json')) as f:
        log = json.load(f)
    if 'codec' in log:
        return codec.restore(model_dir, patch_size=patch_size)
    from ..models import compression
    return getattr(compression, log.get('model', 'TwitterDCN')).restore(model_dir, patch_size=patch_size)


def get_dcn_df(directory, model_directory, write_files=False, force_calc=False):
    """The rate-distortion points of every trained DCN under `model_directory` (one per progress.json) over the images of
    `directory` as a pandas DataFrame, saved as <directory>/dcn-<last component of model_directory>.csv; if that file exists it is
    read and returned instead."""
    import pandas as pd
    name = [x for x in os.path.normpath(str(model_directory)).split(os.sep) if len(x) > 0][-1]
    df_path = os.path.join(directory, 'dcn-{}.csv'.format(name))
    if os.path.isfile(df_path) and not force_calc:
        return pd.read_csv(df_path, index_col=False, float_precision='round_trip')
    files, batch_x = _load(directory)
    rows = []
    for log in sorted(Path(model_directory).glob('**/progress.json')):
        model_dir = os.path.split(str(log))[0]
        dcn = _restore_dcn(model_dir, batch_x.shape[1])
        h = dcn._h
        stats = {k: [] for k in ('ssim', 'psnr', 'entropy', 'bytes', 'bpp', 'msssim')}
        for i in range(0, len(files), DCN_BATCH):
            batch_y, s = codec.compress_n_stats(batch_x[i:i + DCN_BATCH], dcn)
            for k in ('ssim', 'psnr', 'entropy', 'bytes', 'bpp'):
                stats[k].extend(np.atleast_1d(s[k]).tolist())
            stats['msssim'].extend(np.atleast_1d(metrics.msssim(batch_x[i:i + DCN_BATCH], batch_y)).tolist())
            if write_files:
                for j, filename in enumerate(files[i:i + DCN_BATCH]):
                    _write_png(directory, filename, dcn.model_code.replace('/', '-') + '.png', batch_y[j])
        for image_id, filename in enumerate(files):
            with np.errstate(divide='ignore'):
                msssim_db = -10 * np.log10(1 - stats['msssim'][image_id])
            rows.append({'image_id': image_id, 'filename': filename,
                         'model_dir': os.path.relpath(model_dir, str(model_directory)).replace(dcn.scoped_name, ''),
                         'codec': dcn.model_code, 'ssim': stats['ssim'][image_id], 'psnr': stats['psnr'][image_id],
                         'msssim': stats['msssim'][image_id], 'msssim_db': msssim_db, 'entropy': stats['entropy'][image_id],
                         'bytes': int(stats['bytes'][image_id]), 'bpp': stats['bpp'][image_id],
                         'layers': h.n_layers if 'n_layers' in h else None,
                         'quantization': '{}-{:.0f}bpf'.format(h.rounding, h.latent_bpf), 'entropy_reg': h.entropy_weight,
                         'codebook': h.rounding, 'latent': dcn.n_latent, 'latent_shape': '{}x{}x{}'.format(*dcn.latent_shape[-3:]),
                         'n_features': dcn.latent_shape[-1]})
    df = pd.DataFrame(rows, columns=DCN_COLUMNS)
    df.to_csv(df_path, index=False)
    return df
