"""ctypes binding of libssg_hip.so, read from the headers the library ships with.

include/ssg_hip.h and include/similarity.h are the contract, and this module states none of it a second time:
``read_header`` turns their declarations into ``PROTOTYPES`` (name -> (restype, [argtypes])), the declarations inside
``#ifdef SSG_PROFILE`` into ``PROF_PROTOTYPES`` (libssg_hip_prof.so only) and the ``#define SSG_<NAME> <integer>`` lines
into ``CONSTANTS``, at import, with ``re`` and ``ctypes`` alone.  A declaration it cannot type raises, with the
function's name and the text: nothing defaults to a pointer or an int.

The shared library is built in-tree by ``ssl_amd._lib.build()`` (hipcc,
--offload-arch=gfx950; cross-compiles without a GPU) and travels with the
source tree.  There is NO fallback: if the library is missing or a symbol is
absent, importing the compute path raises.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(CSRC, "libssg_hip.so")
# the same sources with -DSSG_PROFILE: kernel-phase ablations + ssg_set_profile_mask (bench.py's per-kernel timings,
# tools/); the product library above has neither
PROF_SO_PATH = os.path.join(CSRC, "libssg_hip_prof.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "ssg_hip.h")
# the reference operator's own (void, stream-less) interface and ssg_last_status
REF_HEADER = os.path.join(os.path.dirname(HEADER), "similarity.h")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "unsigned": ctypes.c_uint, "ssg_stream_t": ctypes.c_void_p}
_RETURNS = dict(_SCALARS, **{"void": None, "const char *": ctypes.c_char_p})


def _argtype(name, param):
    """the ctypes type of one parameter, `T name`, `T *name` or `T name[N]`, of the declaration of `name`"""
    if "*" in param and "(" not in param:
        return ctypes.c_void_p
    m = re.fullmatch(r"(?:const )?(\w+) \w+ ?(\[ ?\d* ?\])?", param)
    if not m or m.group(1) not in _SCALARS:
        raise TypeError(f"ssl_amd._lib: cannot type parameter {param!r} of {name}")
    return ctypes.POINTER(_SCALARS[m.group(1)]) if m.group(2) else _SCALARS[m.group(1)]


def _declarations(text):
    """name -> (restype, [argtypes]) of the `ssg_*` functions a comment-free piece of a header declares"""
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                        # the preprocessor's lines
    text = re.sub(r"\btypedef\b[^;{]*(\{[^}]*\}[^;]*)?;", "", text)              # types, a struct's members included
    text = re.sub(r'\bextern\s+"C"\s*\{|^\s*\}\s*$', "", text, flags=re.M)     # the linkage block's braces
    table = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", stmt)
        if not m:
            raise TypeError(f"ssl_amd._lib: not a function declaration: {stmt!r}")
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if not name.startswith("ssg_"):
            continue                                                          # similarity.h's C++-linkage pair: CXX_SYMBOLS
        if ret not in _RETURNS:
            raise TypeError(f"ssl_amd._lib: unknown return type {ret!r} of {name}")
        if name in table:
            raise TypeError(f"ssl_amd._lib: {name} is declared twice")
        table[name] = (_RETURNS[ret], [] if params == "void" else [_argtype(name, p.strip()) for p in params.split(",")])
    return table


def read_header(text):
    """(prototypes, profiling-build prototypes, constants) of a C header in the style of include/ssg_hip.h."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m.group(1): int(m.group(2).strip("()"))
                 for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SSG_\w+)[ \t]+(\(-?\d+\)|-?\d+)[ \t]*$", text, re.M)}
    prof = r"^[ \t]*#[ \t]*ifdef[ \t]+SSG_PROFILE\b(.*?)^[ \t]*#[ \t]*endif\b"
    inside = "".join(re.findall(prof, text, flags=re.M | re.S))
    return _declarations(re.sub(prof, "", text, flags=re.M | re.S)), _declarations(inside), constants


PROTOTYPES, PROF_PROTOTYPES, CONSTANTS = {}, {}, {}       # PROF_PROTOTYPES: libssg_hip_prof.so only
for _path in (HEADER, REF_HEADER):
    if not os.path.exists(_path):
        raise RuntimeError(f"{_path} is missing: ssl_amd binds libssg_hip.so from its headers")
    with open(_path) as _f:
        for _table, _part in zip((PROTOTYPES, PROF_PROTOTYPES, CONSTANTS), read_header(_f.read())):
            _table.update(_part)
# C++-linkage symbols of include/similarity.h (Itanium mangling of the reference's declarations, similarity.h:2-23)
CXX_SYMBOLS = ("_Z19_compute_similarityPKfPKiPfiiiiii", "_Z28_compute_similarity_backwardPKfS0_PKiPfiiiiii")


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into csrc/libssg_hip.so (+ the profiling build libssg_hip_prof.so)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or out.returncode:
        print(out.stdout)
    if out.returncode:
        raise RuntimeError("building libssg_hip.so failed (see output above)")
    return SO_PATH


_lib = None
_prof = None


def _load(path, prototypes):
    # torch bundles its own HIP runtime (libamdhip64 of its ROCm build).  It must be the one
    # already mapped when libssg_hip.so resolves its libamdhip64 dependency, otherwise the
    # process ends up with two runtimes and our launches see "no ROCm-capable device".
    import torch  # noqa: F401
    if torch.cuda.is_available():
        torch.cuda.init()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ssl_amd/csrc`).  ssl_amd has no CPU / PyTorch fallback for the SSG kernels.")
    L = ctypes.CDLL(path)
    for name, (res, args) in prototypes.items():
        fn = getattr(L, name)  # AttributeError if the symbol is absent: loud by design
        fn.restype = res
        fn.argtypes = args
    for name in CXX_SYMBOLS:
        getattr(L, name)
    return L


def lib():
    """The loaded library with typed prototypes.  Raises if it is not built."""
    global _lib
    if _lib is None:
        _lib = _load(SO_PATH, PROTOTYPES)
    return _lib


def lib_prof():
    """The PROFILING build (libssg_hip_prof.so): same entry points + ssg_set_profile_mask.  For timing tools only."""
    global _prof
    if _prof is None:
        _prof = _load(PROF_SO_PATH, dict(PROTOTYPES, **PROF_PROTOTYPES))
    return _prof


class profile_build:
    """`with _lib.profile_build() as L:` -- inside the block lib() returns the profiling build, so that the engine's
    host code (which calls lib()) runs on it; the product library is restored on exit."""

    def __enter__(self):
        global _lib
        self._saved = _lib
        _lib = lib_prof()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib.ssg_set_profile_mask(0)
        _lib = self._saved
        return False


def check(status):
    if status != 0:
        raise RuntimeError(f"libssg_hip: {lib().ssg_status_string(status).decode()} (status {status})")
