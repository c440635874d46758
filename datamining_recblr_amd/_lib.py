"""ctypes binding of the C-ABI in include/recblr_hip.h.

The shared library is built in-tree by ``datamining_recblr_amd.build`` (or
``__graft_entry__.build()``) as ``datamining_recblr_amd/lib/libdmrecblr.so``.
There is no fallback: if the library is missing, every product entry point
raises ``RecBLRNativeError``.

The headers are the only statement of the prototypes and constants: the
``*SIGNATURES`` tables, ``ABI_VERSION``, ``RB_TILE`` and ``RB_EINVAL`` are
parsed from them on import (``parse_header``).  A new entry point is declared
in the header and defined in csrc/capi.hip, and ``RB_ABI_VERSION`` is bumped;
nothing here is edited.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# RECBLR_LIB points at an alternative build of the same sources (A/B timing
# of compile-time variants, e.g. tools/ab_build.sh); the default is the in-tree build
LIB_PATH = os.environ.get("RECBLR_LIB") or os.path.join(_HERE, "lib", "libdmrecblr.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "recblr_hip.h")


class RecBLRNativeError(RuntimeError):
    """The HIP extension is missing, failed to load, or a kernel call failed."""


# the only types the headers may pass by value (device pointers are passed as integers)
_BY_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
             "float": ctypes.c_float, "double": ctypes.c_double}
_NOT_DECLARATIONS = re.compile(
    r'/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*|\btypedef\b(?:[^;{]|\{[^}]*\})*;|extern\s+"C"\s*\{|^\s*\}\s*$',
    re.S | re.M)


def parse_header(text: str) -> dict:
    """name -> (restype, [argtypes]) of every function a C header declares, in
    declaration order.  Comments, preprocessor lines, typedefs and the
    extern "C" braces are dropped; what remains must be plain declarations,
    one per ';', over pointers and the scalar types of _BY_VALUE."""
    out = {}
    for decl in _NOT_DECLARATIONS.sub(" ", text).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)", decl)
        if m is None:
            raise RecBLRNativeError(f"header: not a plain function declaration: {decl!r}")
        ret, name, params = m.groups()
        if re.fullmatch(r"const\s+char\s*\*", ret):
            restype = ctypes.c_char_p
        elif ret in _BY_VALUE:
            restype = _BY_VALUE[ret]
        else:
            raise RecBLRNativeError(f"header: {name}: unsupported return type {ret!r}")
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            words = param.split()
            by_value = " ".join(words[:-1] if len(words) > 1 else words)   # drop the name
            if "*" in param:
                argtypes.append(ctypes.c_void_p)
            elif by_value in _BY_VALUE:
                argtypes.append(_BY_VALUE[by_value])
            else:
                raise RecBLRNativeError(f"header: {name}: unsupported parameter {param.strip()!r}")
        out[name] = (restype, argtypes)
    return out


def _read(path: str) -> str:
    with open(path) as f:
        return f.read()


def _define(text: str, name: str) -> int:
    m = re.search(rf"^[ \t]*#[ \t]*define[ \t]+{name}[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)
    if m is None:
        raise RecBLRNativeError(f"header: no integer #define {name}")
    return int(m.group(1))


_header = _read(HEADER_PATH)
RB_EINVAL = _define(_header, "RB_EINVAL")
RB_TILE = _define(_header, "RB_TILE")
ABI_VERSION = _define(_header, "RB_ABI_VERSION")

# name -> (restype, argtypes), in header order
SIGNATURES = parse_header(_header)
# the all-position training loss (include/recblr_dense.h): more entry points of
# the same product library, typed with it by load()
DENSE_SIGNATURES = parse_header(_read(os.path.join(os.path.dirname(HEADER_PATH),
                                                   "recblr_dense.h")))
# the sampled pairwise loss (include/recblr_pairs.h): likewise
PAIR_SIGNATURES = parse_header(_read(os.path.join(os.path.dirname(HEADER_PATH),
                                                  "recblr_pairs.h")))
# candidate-list scoring (include/recblr_candidates.h): likewise
CANDIDATE_SIGNATURES = parse_header(_read(os.path.join(os.path.dirname(HEADER_PATH),
                                                       "recblr_candidates.h")))
# catalogue filters (include/recblr_filters.h): likewise
FILTER_SIGNATURES = parse_header(_read(os.path.join(os.path.dirname(HEADER_PATH),
                                                    "recblr_filters.h")))
# diversity caps (include/recblr_groups.h): likewise
GROUP_SIGNATURES = parse_header(_read(os.path.join(os.path.dirname(HEADER_PATH),
                                                   "recblr_groups.h")))
# score priors (include/recblr_priors.h): likewise
PRIOR_SIGNATURES = parse_header(_read(os.path.join(os.path.dirname(HEADER_PATH),
                                                   "recblr_priors.h")))
# the experimental library (experimental/recblr_exp.h: opt-in kernels that
# measured slower than the default path; never loaded unless requested)
EXP_SIGNATURES = parse_header(_read(os.path.join(_HERE, "experimental", "recblr_exp.h")))
# the probe library (probes/recblr_probe.h: bench.py's measurement aids)
PROBE_SIGNATURES = parse_header(_read(os.path.join(_HERE, "probes", "recblr_probe.h")))
# the session library (session/recblr_session.h: the one-launch per-event
# encoder step of session.py; loaded on the first step)
SESSION_SIGNATURES = parse_header(_read(os.path.join(_HERE, "session", "recblr_session.h")))

_lock = threading.Lock()
_loaded = {}


def _load(path, signatures, missing, version=None, mismatch=None, cache=True,
          hint="") -> ctypes.CDLL:
    """Load (once per path when cached) a library and type its prototypes."""
    with _lock:
        if cache and path in _loaded:
            return _loaded[path]
        if not os.path.exists(path):
            raise RecBLRNativeError(f"{missing}: {path} is missing. Run "
                                    f"`python -m datamining_recblr_amd.build`{hint}.")
        try:
            lib = ctypes.CDLL(path)
        except OSError as exc:  # pragma: no cover - depends on the host
            raise RecBLRNativeError(f"failed to load {path}: {exc}") from exc
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if version is not None and getattr(lib, version)() != ABI_VERSION:
            raise RecBLRNativeError(mismatch.format(getattr(lib, version)(), ABI_VERSION))
        if cache:
            _loaded[path] = lib
        return lib


def load(path: str | None = None) -> ctypes.CDLL:
    """Load (once) and return the native library with typed prototypes.  An
    explicit path is loaded afresh and not cached."""
    return _load(path or LIB_PATH,
                 {**SIGNATURES, **DENSE_SIGNATURES, **PAIR_SIGNATURES, **CANDIDATE_SIGNATURES,
                  **FILTER_SIGNATURES, **GROUP_SIGNATURES, **PRIOR_SIGNATURES},
                 "HIP extension not built",
                 "rb_version",
                 "ABI mismatch: library {} vs binding {}; rebuild", cache=path is None,
                 hint=" (hipcc --offload-arch=gfx950)")


def load_probe() -> ctypes.CDLL:
    """The probe library (lib/libdmrecblr_probe.so): measurement aids for
    bench.py, never on the model's path."""
    return _load(os.path.join(os.path.dirname(LIB_PATH), "libdmrecblr_probe.so"),
                 PROBE_SIGNATURES, "probe library not built")


def load_exp() -> ctypes.CDLL:
    """The experimental library (lib/libdmrecblr_exp.so, experimental/
    recblr_exp.h): the opt-in fused GatedRecurrentLayer kernels.  Loaded only
    when one of them is requested; the default path never loads it."""
    return _load(os.path.join(os.path.dirname(LIB_PATH), "libdmrecblr_exp.so"), EXP_SIGNATURES,
                 "experimental library not built", "rb_exp_version",
                 "experimental library ABI {} vs {}; rebuild")


def load_session() -> ctypes.CDLL:
    """The session library (lib/libdmrecblr_session.so, session/
    recblr_session.h): stateful per-event inference (session.py)."""
    return _load(os.path.join(os.path.dirname(LIB_PATH), "libdmrecblr_session.so"),
                 SESSION_SIGNATURES, "session library not built", "rb_session_version",
                 "session library ABI {} vs {}; rebuild")


_fns = {}
_failure_hooks = []


def on_failure(hook) -> None:
    """Register hook() to run whenever a C-ABI call returns an error (device
    state cached by the Python side, e.g. the column sums' ticket counters,
    is dropped rather than trusted after a failure)."""
    _failure_hooks.append(hook)


def _check(rc: int, name: str, lib: ctypes.CDLL, last_error: str, hooks: bool = True) -> None:
    """Raise on a non-zero status with the library's message for it."""
    if rc == 0:
        return
    kind = str(rc)
    if hooks:
        for hook in _failure_hooks:
            hook()
        kind = "invalid argument" if rc == RB_EINVAL else f"hipError {rc}"
    msg = getattr(lib, last_error)()
    raise RecBLRNativeError(f"{name} failed ({kind}): {msg.decode() if msg else ''}")


def call(name: str, *args) -> None:
    """Invoke a C-ABI entry point and raise on a non-zero status."""
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    rc = fn(*args)
    if rc != 0:
        _check(rc, name, load(), "rb_last_error_string")


def call_probe(name: str, *args) -> None:
    """Invoke a probe-library entry point and raise on a non-zero status (the
    bare status, and no failure hooks: nothing on the model's path ran)."""
    lib = load_probe()
    _check(getattr(lib, name)(*args), name, lib, "rb_probe_last_error_string", hooks=False)


def call_exp(name: str, *args) -> None:
    """Invoke an experimental-library entry point and raise on a non-zero status."""
    lib = load_exp()
    _check(getattr(lib, name)(*args), name, lib, "rb_exp_last_error_string")


def call_session(name: str, *args) -> None:
    """Invoke a session-library entry point and raise on a non-zero status."""
    lib = load_session()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        _check(rc, name, lib, "rb_session_last_error_string")
