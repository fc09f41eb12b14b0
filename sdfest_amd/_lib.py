"""ctypes binding of libsdfr_hip.so, derived from its C ABI header include/sdfr.h.

The shared library is built in-tree by ``sdfest_amd/csrc/Makefile`` (see
``__graft_entry__.build``).  There is NO fallback: if the library is missing
or a call fails, the error is raised -- the product never computes on the CPU.

The header is the binding's one source: at import, every ``SDFR_API`` declaration becomes an entry of
``SIGNATURES`` and every integer ``#define`` an entry of ``ABI``.  A type or a macro that cannot be read
raises, so a new declaration is never bound wrong unnoticed.
"""
import ast
import ctypes
import operator
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "sdfr.h")
# SDFR_LIB: another build of the same library (timing experiments: tools/microbench/build_variant.sh)
LIB_PATH = os.environ.get("SDFR_LIB") or os.path.join(_HERE, "libsdfr_hip.so")
_lib = None

# by-value C types of the ABI; any pointer is c_void_p, a returned `const char*` c_char_p, a returned `void` None
_CTYPES = {
    "int": ctypes.c_int,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "size_t": ctypes.c_size_t,
    "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong,
}
_C_WORDS = {"const", "signed", "unsigned", "char", "short", "int", "long", "float", "double", "void"}
_NOT_CONSTANTS = {"SDFR_H_", "SDFR_API"}   # the include guard and the export attribute
_INT_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.LShift: operator.lshift,
            ast.BitOr: operator.or_, ast.USub: operator.neg}


def _ctype(ctype: str, func: str, returned: bool = False):
    words = ctype.replace("*", " * ").split()
    if returned and words == ["const", "char", "*"]:
        return ctypes.c_char_p
    if "*" in words:
        return ctypes.c_void_p
    if returned and words == ["void"]:
        return None
    t = _CTYPES.get(" ".join(w for w in words if w != "const"))
    if t is None:
        raise ValueError(f"{func}: no ctypes type for the C type '{ctype.strip()}'")
    return t


def _param(param: str, func: str):
    m = re.fullmatch(r"([\w\s*]*[\s*])([A-Za-z_]\w*)", param.strip())
    if not m or m.group(2) in _C_WORDS:
        raise ValueError(f"{func}: parameter '{param.strip()}' has no name")
    return _ctype(m.group(1), func)


def _int_expr(node, known: dict) -> int:
    if isinstance(node, ast.Constant) and type(node.value) is int:
        return node.value
    if isinstance(node, ast.Name):
        return known[node.id]
    if isinstance(node, ast.UnaryOp) and type(node.op) in _INT_OPS:
        return _INT_OPS[type(node.op)](_int_expr(node.operand, known))
    if isinstance(node, ast.BinOp) and type(node.op) in _INT_OPS:
        return _INT_OPS[type(node.op)](_int_expr(node.left, known), _int_expr(node.right, known))
    raise ValueError(ast.dump(node))


def parse_header(text: str):
    """(signatures, constants) of the C ABI header `text`: {name: (restype, [argtypes])} of every ``SDFR_API``
    declaration, and {name: int} of every ``#define`` but the include guard and ``SDFR_API``.  A macro's value is
    an integer literal (decimal or hex, optional ``u``) or an expression of such literals and earlier macros."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", text, re.M):
        if name in _NOT_CONSTANTS:
            continue
        try:
            expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uU]\b", r"\1", value.strip())
            constants[name] = _int_expr(ast.parse(expr, mode="eval").body, constants)
        except (SyntaxError, ValueError, KeyError):
            raise ValueError(f"#define {name}{value}: not an integer constant expression") from None
    signatures = {}
    declarations = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for decl in re.findall(r"\bSDFR_API\b([^;]*);", declarations):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(sdfr_\w+)\s*\(([^()]*)\)\s*", decl)
        if not m:
            raise ValueError(f"cannot read the declaration 'SDFR_API {' '.join(decl.split())};'")
        ret, func, params = m.groups()
        args = [] if params.strip() == "void" else [_param(p, func) for p in params.split(",")]
        signatures[func] = (_ctype(ret, func, returned=True), args)
    return signatures, constants


def _read_header():
    try:
        with open(HEADER) as f:
            return parse_header(f.read())
    except FileNotFoundError:
        raise ImportError(f"{HEADER} not found: sdfest_amd binds libsdfr_hip.so from this header and must be "
                          "imported from the repository tree") from None


SIGNATURES, ABI = _read_header()


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `make -C sdfest_amd/csrc` "
                "(or __graft_entry__.build()); sdfest_amd has no CPU fallback")
        import torch  # noqa: F401  loads torch's libamdhip64 first so both share one HIP runtime
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().sdfr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def workspace(nbytes: int, what: str, device, given=None):
    """The workspace of a call whose ``*_workspace_bytes`` function `what` returned `nbytes`: 0 means that it refused
    the arguments, which raises as a failed call does; otherwise `given` (a buffer the caller made beforehand) or a new
    uint8 device tensor of that size."""
    if nbytes == 0:
        check(ABI["SDFR_E_INVALID"], what)
    if given is not None:
        return given
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, device=device)
