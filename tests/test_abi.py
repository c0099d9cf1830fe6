"""The C-ABI library loads on a CPU-only box and exports every symbol include/nimg.h declares (no compute calls); the ctypes
binding is derived from that header, and its parser is held to a synthetic header here."""
import ctypes
import os
import re
from ctypes import c_float, c_int, c_long, c_size_t, c_void_p

import pytest

from neural_imaging_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, 'include', 'nimg.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(nimg_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_entry_points():
    syms = _header_symbols()
    assert 'nimg_djpeg_fwd' in syms and 'nimg_conv2d_fwd' in syms and len(syms) >= 30


def test_library_exports_every_declared_symbol():
    assert os.path.isfile(_lib.LIB_PATH), 'build libnimg.so first (__graft_entry__.build())'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in _header_symbols() if not hasattr(lib, s)]
    assert not missing, 'declared in include/nimg.h but not exported: {}'.format(missing)


SYNTHETIC_HEADER = """
/* a block comment that mentions int nimg_not_this(int a); and
 * runs over two lines */
#ifndef NIMG_H
#define NIMG_H
#include <stddef.h>
extern "C" {
#define NIMG_OK 0
#define NIMG_ERR_ARG (-1)   /* a trailing comment
                             * that runs on, #define NIMG_NOT_THIS 5
                             */
#define NIMG_TICKET_BYTES (64 * 1024)
#define NIMG_HEX 0x10 // sixteen
#define NIMG_EXPR (1 << 4)
#define NIMG_NAME nimg_version
// int nimg_x(int commented_out);
int nimg_version(void);
size_t nimg_bytes(int n, long count);       // size_t return
long nimg_count( void );
int nimg_three_lines(const float* x, float* y /* may be NULL */, const float* const* parts,
                     unsigned char* bytes, void** out, int n, long total, size_t workspace_bytes,
                     float alpha, void* stream);
const float* nimg_table(int);
}
#endif
"""


def test_parser_reads_a_synthetic_header():
    P = c_void_p
    assert _lib.parse_prototypes(SYNTHETIC_HEADER) == {
        'nimg_version': (c_int, []),
        'nimg_bytes': (c_size_t, [c_int, c_long]),
        'nimg_count': (c_long, []),
        'nimg_three_lines': (c_int, [P, P, P, P, P, c_int, c_long, c_size_t, c_float, P]),
        'nimg_table': (P, [c_int]),
    }
    # integer literals, a parenthesised negative and a product of literals; anything else (a shift, a name) is not a constant
    assert _lib.parse_constants(SYNTHETIC_HEADER) == {'NIMG_OK': 0, 'NIMG_ERR_ARG': -1, 'NIMG_TICKET_BYTES': 65536,
                                                      'NIMG_HEX': 16}


@pytest.mark.parametrize('declaration', ['int nimg_bad(double x);', 'int nimg_bad(int n, int64_t count, void* stream);',
                                         'int nimg_bad(unsigned int n);', 'int nimg_bad(long long);',
                                         'double nimg_bad(int n);', 'void nimg_bad(int n);'])
def test_parser_refuses_an_unknown_scalar_type(declaration):
    with pytest.raises(ValueError, match='nimg_bad'):
        _lib.parse_prototypes('int nimg_good(int n);\n' + declaration)


def test_python_prototypes_cover_the_header():
    syms = set(_header_symbols())       # every nimg_name( outside a block comment, found without the binding's parser
    assert syms == set(_lib.PROTOTYPES.keys()), syms ^ set(_lib.PROTOTYPES.keys())
    for name, (res, args) in _lib.PROTOTYPES.items():
        assert res in (c_int, c_long, c_size_t, c_float, c_void_p), name
        assert all(a in (c_int, c_long, c_size_t, c_float, c_void_p) for a in args), name
    assert _lib.PROTOTYPES['nimg_abi_version'] == (c_int, [])
    assert _lib.PROTOTYPES['nimg_bias_grad'] == (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_size_t, c_void_p])
    assert _lib.PROTOTYPES['nimg_isp_residual_workspace_bytes'] == (c_long, [])
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'nimg.h')).read()
    declared = int(re.search(r'#define\s+NIMG_ABI_VERSION\s+(\d+)', header).group(1))
    assert lib.nimg_abi_version() == declared == _lib.ABI_VERSION       # library, header and binding agree (load() checks too)


def _header_defines():
    header = open(os.path.join(ROOT, 'include', 'nimg.h')).read()
    return {name: int(value.strip('()')) for name, value in re.findall(r'#define\s+(NIMG_\w+)\s+(\d+|\(-\d+\))\s', header)}


def test_constants_come_from_the_header():
    from neural_imaging_amd import ops
    defines = _header_defines()
    for name in ('BF16_IN', 'BF16_OUT', 'BF16_MASK', 'BF16_DZ', 'D2S_OUT', 'S2D_OUT', 'COPY_LRELU', 'MASK_CONV'):
        value = getattr(ops, name)
        assert type(value) is int and value == defines['NIMG_' + name] == _lib.CONSTANTS['NIMG_' + name], name
    assert ops.ROUNDING == {mode: defines['NIMG_ROUND_' + mode.upper()]
                            for mode in ('round', 'soft', 'sin', 'harmonic', 'identity')}
    assert set(_lib.ERRORS) == {defines['NIMG_ERR_ARG'], defines['NIMG_ERR_LAUNCH'], defines['NIMG_ERR_WORKSPACE']} == {-1, -2, -3}
    assert _lib.ABI_VERSION == defines['NIMG_ABI_VERSION'] and _lib.TICKET_BYTES == _lib.CONSTANTS['NIMG_TICKET_BYTES'] == 64 * 1024


def test_no_oracle_import_in_product():
    """The product path must never route through the oracle or a CPU fallback."""
    pkg = os.path.join(ROOT, 'neural-imaging_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M), os.path.join(dirpath, f)
