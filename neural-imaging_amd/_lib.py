"""
ctypes binding of libnimg.so, derived at import from the C ABI's one written copy, include/nimg.h.

The library is built in-tree by neural-imaging_amd/csrc/build.sh (hipcc --offload-arch=gfx950).  There is NO
fallback: if the header or the library is missing, or an entry point returns an error code, a RuntimeError is raised.
"""
import ctypes
import os
import re
from ctypes import c_float, c_int, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NIMG_LIBPATH') or os.path.join(_HERE, 'libnimg.so')     # override: A/B of kernel builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'nimg.h')            # the file csrc/common.h includes

P = c_void_p  # every device pointer / stream is passed as an opaque pointer

_SCALARS = {'int': c_int, 'long': c_long, 'size_t': c_size_t, 'float': c_float}    # extend on purpose, never by guessing
_TYPE_WORDS = set(_SCALARS) | {'unsigned', 'signed', 'short', 'char', 'double', 'void'}      # never a parameter's name
_DECLARATION = re.compile(r'([A-Za-z_][\w\s\*]*?)\b(nimg_\w+)\s*\(([^()]*)\)\s*;')
_LITERAL = r'0[xX][0-9a-fA-F]+|\d+'
_DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+(NIMG_\w+)[ \t]+'
                     r'(?:({0})|\([ \t]*(-?[ \t]*(?:{0}))[ \t]*\)|\([ \t]*((?:{0})(?:[ \t]*\*[ \t]*(?:{0}))+)[ \t]*\))[ \t]*$'
                     .format(_LITERAL), re.M)


def _strip_comments(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))


def _ctype(spelling, named, where):
    """ctypes type of one C parameter (`named`: the last word is its name) or of a return type."""
    if '*' in spelling:
        return P
    words = [w for w in spelling.split() if w != 'const']
    if named and len(words) == 2 and words[1] not in _TYPE_WORDS:
        words.pop()
    if len(words) != 1 or words[0] not in _SCALARS:
        raise ValueError('include/nimg.h: no ctypes mapping for "{}" in the declaration of {}'.format(spelling.strip(), where))
    return _SCALARS[words[0]]


def parse_prototypes(text):
    """name -> (restype, argtypes) of every `ret nimg_name(args);` declaration in the header text."""
    code = '\n'.join(l for l in _strip_comments(text).split('\n') if not l.lstrip().startswith('#'))
    protos = {}
    for ret, name, args in _DECLARATION.findall(code):
        params = [] if args.strip() in ('', 'void') else args.split(',')
        protos[name] = (_ctype(ret, False, name), [_ctype(p, True, name) for p in params])
    return protos


def parse_constants(text):
    """NIMG_X -> int of every `#define NIMG_X <value>` whose value is an integer literal, (-literal) or (literal * literal ...)."""
    consts = {}
    for name, plain, negative, product in _DEFINE.findall(_strip_comments(text)):
        value = 1
        for factor in (plain or negative or product).replace(' ', '').replace('\t', '').split('*'):
            value *= int(factor, 0)
        consts[name] = value
    return consts


def _read_header():
    if not os.path.isfile(HEADER_PATH):
        raise RuntimeError('include/nimg.h not found at {} - the binding is derived from it and ships next to the package'
                           .format(HEADER_PATH))
    with open(HEADER_PATH) as f:
        return f.read()


_HEADER = _read_header()
PROTOTYPES = parse_prototypes(_HEADER)          # name -> (restype, argtypes), one entry per declaration of include/nimg.h
CONSTANTS = parse_constants(_HEADER)            # NIMG_X -> int, the header's integer #defines
del _HEADER

ERRORS = {CONSTANTS['NIMG_ERR_ARG']: 'NIMG_ERR_ARG (invalid argument / unsupported configuration)',
          CONSTANTS['NIMG_ERR_LAUNCH']: 'NIMG_ERR_LAUNCH (HIP kernel launch failed)',
          CONSTANTS['NIMG_ERR_WORKSPACE']: 'NIMG_ERR_WORKSPACE (workspace too small)'}

_lib = None


ABI_VERSION = CONSTANTS['NIMG_ABI_VERSION']
TICKET_BYTES = CONSTANTS['NIMG_TICKET_BYTES']


def load():
    """Load libnimg.so (once) and attach prototypes.  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError('libnimg.so not found at {} - build it with neural-imaging_amd/csrc/build.sh '
                           '(or __graft_entry__.build()); there is no CPU fallback'.format(LIB_PATH))
    # torch first: its wheel carries its own copy of the HIP runtime, and libnimg.so must bind to THAT instance (the streams and
    # device pointers it is handed come from it).  Loaded before torch, libnimg.so pulls in /opt/rocm's libamdhip64 as a second
    # runtime and every launch on a torch stream fails (seen as NIMG_ERR_LAUNCH from `python __graft_entry__.py smoke`, whose
    # build() loaded the library before anything had imported torch).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError here == the library lacks an entry point the header declares
        fn.restype = res
        fn.argtypes = args
    if lib.nimg_abi_version() != ABI_VERSION:
        raise RuntimeError('libnimg.so at {} was built with ABI version {}, include/nimg.h now declares {}: the library is '
                           'older than the header - rebuild it (neural-imaging_amd/csrc/build.sh)'
                           .format(LIB_PATH, lib.nimg_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def call(name, *args):
    """Call an int-returning entry point and raise on a non-zero status."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError('{} failed: {}'.format(name, ERRORS.get(rc, rc)))
    return rc
