"""CPU-side checks of the drop-in boundary: the shared library loads, exports every symbol that
include/tome_hip.h declares, and the host logic that needs no GPU (clamping, workspace sizing, argument
validation, loud failure on CPU tensors) behaves.  No kernel is launched here."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(measurement_build=False):
    """Entry points include/tome_hip.h declares: the product ABI, or (measurement_build) what its
    `#ifdef TOME_PROFILE_HOOKS` section adds for lib/libtome_hip_prof.so."""
    text = open(os.path.join(ROOT, "include", "tome_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    hooks = re.findall(r"#ifdef TOME_PROFILE_HOOKS(.*?)#endif", text, flags=re.S)
    product = re.sub(r"#ifdef TOME_PROFILE_HOOKS.*?#endif", "", text, flags=re.S)
    pick = "".join(hooks) if measurement_build else product
    return sorted(set(re.findall(r"\b(tome_[a-z_]+)\s*\(", pick)))


_C_TYPES = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _ctype(decl, ret=False):
    """The ctypes class of one C parameter or return type as include/tome_hip.h spells it (the parameter's name may still
    be on it): any pointer and tome_stream_t are a c_void_p, `const char *` as a return type a c_char_p."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if ret and words[:3] == ["const", "char", "*"] else ctypes.c_void_p
    words = [w for w in words if w != "const"]
    if words[0] == "tome_stream_t":
        return ctypes.c_void_p
    return _C_TYPES[words[0]]


def _declared_prototypes():
    """name -> (restype, [argtypes]) of every product prototype in include/tome_hip.h."""
    text = open(os.path.join(ROOT, "include", "tome_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef TOME_PROFILE_HOOKS.*?#endif", "", text, flags=re.S)
    text = re.sub(r"enum\s+\w+\s*\{.*?\}", "", text, flags=re.S)
    text = re.sub(r"^\s*(#|extern\b|typedef\b|\}).*$", "", text, flags=re.M)
    protos = {}
    for statement in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(tome_[a-z_]+)\s*\(([^)]*)\)\s*", statement)
        if m is None:
            assert "tome_" not in statement, statement
            continue
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        protos[name] = (_ctype(ret, ret=True), [_ctype(p) for p in params])
    return protos


def test_signature_table_agrees_with_the_header():
    """Every row of _abi.SIGNATURES, and what bind() put on the loaded library, is the header's prototype mapped to
    ctypes: an argtypes list that is one int64 short would otherwise bind without complaint and shift a launch's
    arguments."""
    from tome import _abi
    protos = _declared_prototypes()
    assert sorted(protos) == _declared_symbols() == sorted(_abi.SIGNATURES)
    assert _abi.SYMBOLS == tuple(_abi.SIGNATURES)
    L = _abi.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes, argtypes)
        assert _abi.SIGNATURES[name][:2] == (restype, argtypes), name


def test_library_without_a_later_entry_binds_and_says_so_on_use(monkeypatch):
    """A flagged row ("added to ABI v11 later") that the library lacks is skipped by bind(); require_symbol reports it
    when the entry is called.  A row without the flag must be exported: AttributeError at bind."""
    from tome import _abi
    real = ctypes.CDLL(_abi.LIB_PATH)

    class Lacking:
        """libtome_hip.so as a build from before `missing` was added would look to ctypes.CDLL."""
        def __init__(self, *missing):
            self._missing = missing

        def __getattr__(self, name):
            if name in self._missing:
                raise AttributeError(name)
            return getattr(real, name)

    later = [name for name, row in _abi.SIGNATURES.items() if row[2]]
    assert "tome_layernorm_backward" in later and "tome_short_attention_backward" in later
    assert "tome_merge_wavg" not in later and "tome_abi_version" not in later
    for name in later:
        monkeypatch.setattr(ctypes, "CDLL", lambda path, name=name: Lacking(name))
        L = _abi.bind(_abi.LIB_PATH)
        with pytest.raises(_abi.TomeHipError, match=f"{name} is missing from the loaded library.*built before"):
            _abi.require_symbol(L, name)
        other = next(n for n in later if n != name)
        assert _abi.require_symbol(L, other).argtypes == _abi.SIGNATURES[other][1]  # ... and only that one is skipped
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Lacking("tome_merge_wavg"))
    with pytest.raises(AttributeError):
        _abi.bind(_abi.LIB_PATH)


def _size_case(x_dtype=torch.bfloat16):
    return torch.zeros((2, 6, 8), dtype=x_dtype)


def test_prep_size_checks_device_and_shape_and_casts():
    """_abi._prep_size, the size preparation of all four merge_wavg wrappers (called directly, nothing is launched): a
    size on another device than the tokens' is refused -- a host pointer must never reach a kernel --, so is a wrong
    shape; a dtype that is neither the tokens' nor fp32 is cast to the tokens'; None stands for ones of the tokens' dtype."""
    from tome import _abi
    x = _size_case()
    with pytest.raises(_abi.TomeHipError, match="tensor on meta, tokens on cpu"):
        _abi._prep_size(torch.ones((2, 6, 1), device="meta"), 2, 6, x)
    with pytest.raises(_abi.TomeHipError, match="tensor on cpu, tokens on meta"):
        _abi._prep_size(torch.ones((2, 6, 1)), 2, 6, x.to("meta"))
    for bad in ((2, 6), (2, 5, 1), (6, 2, 1), (2, 6, 2)):
        with pytest.raises(_abi.TomeHipError, match="size must be"):
            _abi._prep_size(torch.ones(bad), 2, 6, x)
    for given, want in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.bfloat16),
                        (torch.float64, torch.bfloat16), (torch.int64, torch.bfloat16)):
        size, sdtype = _abi._prep_size(torch.full((2, 6, 1), 3, dtype=given), 2, 6, x)
        assert size.dtype == sdtype == want and size.is_contiguous() and bool((size == 3).all())
    size, sdtype = _abi._prep_size(torch.ones((6, 2, 1)).transpose(0, 1), 2, 6, x)  # a view: made contiguous
    assert size.is_contiguous() and sdtype == torch.float32
    assert _abi._prep_size(None, 2, 6, x) == (None, torch.bfloat16)
    assert _abi._prep_size(None, 2, 6, _size_case(torch.float32)) == (None, torch.float32)


def test_header_symbols_are_exported():
    from tome import _abi
    L = _abi.lib()
    names = _declared_symbols()
    assert len(names) >= 11
    for name in names:
        assert hasattr(L, name), f"{name} declared in include/tome_hip.h but not exported"
    assert set(names) == set(_abi.SYMBOLS)
    assert L.tome_abi_version() == _abi.ABI_VERSION


def test_measurement_hooks_live_in_their_own_library_only():
    """tome_profile_enable / tome_profile_read (stage events + repeated launches for bench.py's roofline figures) are
    not part of the product: libtome_hip.so does not export them, lib/libtome_hip_prof.so (-DTOME_PROFILE_HOOKS,
    bound by bench.py's stage-timing leg alone) exports them beside the whole product ABI."""
    from tome import _abi
    hooks = _declared_symbols(measurement_build=True)
    assert hooks == ["tome_profile_enable", "tome_profile_read"]
    product = ctypes.CDLL(_abi.LIB_PATH)
    prof = ctypes.CDLL(os.path.join(os.path.dirname(_abi.LIB_PATH), "libtome_hip_prof.so"))
    for name in hooks:
        assert not hasattr(product, name) and hasattr(prof, name), name
        assert name not in _abi.SYMBOLS
    for name in _declared_symbols():
        assert hasattr(prof, name), name


def test_effective_r_matches_reference_clamp():
    from tome import _abi
    for T in range(0, 14):
        for r in (-2, 0, 1, 3, 7, 1000):
            for cls in (False, True):
                for dist in (False, True):
                    want = max(0, min(r, (T - cls - dist) // 2))  # merge.py:36-47
                    assert _abi.effective_r(T, r, cls, dist) == want
                    assert _abi.lib().tome_effective_r(T, r, int(cls), int(dist)) == want


def test_workspace_bytes_monotone_and_aligned():
    from tome import _abi
    L = _abi.lib()
    a = L.tome_match_workspace_bytes(8, 1568, 64)
    b = L.tome_match_workspace_bytes(16, 1568, 64)
    assert a % 256 == 0 and b > a
    assert a >= 4 * 8 * 1568 * 64
    assert L.tome_match_workspace_bytes(0, 10, 10) == 0


def test_argument_validation_without_gpu():
    """Bad arguments are rejected before any launch, with a message."""
    from tome import _abi
    L = _abi.lib()
    rc = L.tome_merge(None, 0, 2, 16, 8, 4, None, None, None, 0, 0, None, None, None)
    assert rc == 1 and b"tome_merge" in L.tome_last_error()
    rc = L.tome_match(None, 0, 2, 16, 8, 128, 8, 4, 0, 0, None, None, None, None, None, None, 0, None)
    assert rc == 1
    buf = ctypes.create_string_buffer(64)
    rc = L.tome_merge_wavg(buf, 7, None, 0, 1, 8, 4, 9, buf, buf, buf, 0, None, buf, buf, None, None)
    assert rc == 1  # r outside (0, T/2]


def test_cpu_tensors_fail_loudly():
    from tome import _abi, merge as tm
    with pytest.raises(_abi.TomeHipError, match="no CPU path"):
        tm.bipartite_soft_matching(torch.randn(1, 8, 4), 2)


def test_missing_library_fails_loudly(monkeypatch):
    from tome import _abi
    monkeypatch.setattr(_abi, "_lib", None)
    monkeypatch.setattr(_abi, "LIB_PATH", "/nonexistent/libtome_hip.so")
    with pytest.raises(_abi.TomeHipError, match="no fallback"):
        _abi.lib()


def test_parse_r_golden(golden_dir):
    import json
    from tome.utils import parse_r
    for e in json.load(open(os.path.join(golden_dir, "parse_r.json"))):
        r = tuple(e["r"]) if e["r_type"] == "tuple" else e["r"]
        assert parse_r(e["num_layers"], r) == e["out"]


def test_product_never_imports_oracle():
    """The product package must not reference the oracle (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "video-how-do-your-tokens-merge_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), (dirpath, f)
