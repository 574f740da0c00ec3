"""The C-ABI library loads (no GPU needed) and exports every symbol include/cdx.h declares; binding struct layouts
match the library's sizeof; both ctypes tables (_native._SIGS, _host._SIGS) agree with the C text in names, arity and
argument classes.  CPU only."""
import ctypes as C
import os
import re

from tests.conftest import REPO

# C scalar type → the ctypes that may bind it (int and int32_t are the same size on this ABI; the tables mix them)
SCALARS = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "int64_t": (C.c_int64,),
           "uint64_t": (C.c_uint64,), "size_t": (C.c_size_t,), "double": (C.c_double,)}


def prototypes(src, prefix, end):
    """{name: (return type, [parameter types])} of the C functions named ``prefix*`` in ``src``: declarations
    (end ";") or definitions (end "{").  Comments go first; types lose ``const`` and the parameter's name."""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)

    def ctype(text, named):
        text = " ".join(text.replace("*", " * ").split())
        if named and text != "void":
            text = text.rsplit(" ", 1)[0]
        return re.sub(r"\bconst ", "", text).replace(" *", "*")
    out = {}
    pattern = r"^\s*((?:const\s+)?\w+[\s*]+)(%s\w+)\s*\(([^()]*)\)\s*%s" % (prefix, re.escape(end))
    for ret, name, params in re.findall(pattern, src, flags=re.M):
        types = [ctype(p, True) for p in params.split(",") if p.strip()]
        out[name] = (ctype(ret, False), [] if types == ["void"] else types)
    return out


def header_prototypes():
    return prototypes(open(os.path.join(REPO, "include", "cdx.h")).read(), "cdx_", ";")


def host_prototypes():
    """The definitions inside host_ref.cpp's extern "C" block."""
    src = open(os.path.join(REPO, "compliancedex_amd", "csrc", "host_ref.cpp")).read()
    return prototypes(src.split('extern "C" {', 1)[1].rsplit('}  // extern "C"', 1)[0], "cdxh_", "{")


def _binds(ctype, bound):
    """A C type against the ctypes class bound to it (None: void)."""
    if ctype == "void":
        return bound is None
    if bound is None:
        return False
    if ctype == "cdx_stream_t":
        return bound is C.c_void_p
    if ctype.endswith("*"):
        if bound is C.c_void_p or (bound is C.c_char_p and ctype == "char*"):
            return True
        if not issubclass(bound, C._Pointer):
            return False
        to, base = bound._type_, ctype[:-1]
        if issubclass(to, C.Structure):  # POINTER(CdxFooBar) ↔ cdx_foo_bar*
            return re.sub(r"(?<!^)(?=[A-Z])", "_", to.__name__).lower() == base
        return to in SCALARS.get(base, ())
    return bound in SCALARS.get(ctype, ())


def abi_mismatches(protos, sigs):
    """[(function, where)] for every disagreement of a ctypes table {name: (restype, argtypes)} with parsed C
    prototypes: "unbound" (declared, not in the table), "undeclared" (in the table, not in the C text), "arity",
    "return" or "arg <index>"."""
    bad = [(n, "unbound") for n in sorted(set(protos) - set(sigs))]
    bad += [(n, "undeclared") for n in sorted(set(sigs) - set(protos))]
    for name in sorted(set(protos) & set(sigs)):
        (ret, params), (res, args) = protos[name], sigs[name]
        if not _binds(ret, res):
            bad.append((name, "return"))
        if len(params) != len(args):
            bad.append((name, "arity"))
            continue
        bad += [(name, f"arg {i}") for i, (c, a) in enumerate(zip(params, args)) if not _binds(c, a)]
    return bad


def declared_functions():
    return sorted(header_prototypes())


def test_header_declares_the_path():
    names = declared_functions()
    for n in ("cdx_gpis_mean", "cdx_gpis_std", "cdx_fk_forward", "cdx_fk_backward", "cdx_closure",
              "cdx_sdf_forward", "cdx_sdf_backward"):
        assert n in names


def test_native_table_matches_the_header():
    from compliancedex_amd import _native
    protos = header_prototypes()
    assert len(protos) == len(_native._SIGS) >= 101
    assert abi_mismatches(protos, _native._SIGS) == []


def test_host_table_matches_host_ref():
    """A cdxh_* function without its line in _host._SIGS, or whose line has another arity or argument class than its
    definition, fails here."""
    from compliancedex_amd import _host
    protos = host_prototypes()
    assert len(protos) == len(_host._SIGS) >= 38
    assert abi_mismatches(protos, _host._SIGS) == []


def test_abi_checker_can_fail():
    """A dropped last argument, a c_int64 bound as c_int32 and a removed entry are reported, and nothing else."""
    from compliancedex_amd import _host
    sigs = {k: (r, list(a)) for k, (r, a) in _host._SIGS.items()}
    sigs["cdxh_hand_cost"][1].pop()
    at = sigs["cdxh_knn"][1].index(C.c_int64)
    sigs["cdxh_knn"][1][at] = C.c_int32
    del sigs["cdxh_svd3"]
    assert abi_mismatches(host_prototypes(), sigs) == [("cdxh_svd3", "unbound"), ("cdxh_hand_cost", "arity"),
                                                        ("cdxh_knn", f"arg {at}")]
    # the parser on text of its own: a pointer bound as an integer, a wrong struct, a wrong return, an extra entry
    protos = prototypes("int f_a(const cdx_chain* c, double* x);  /* int f_no(void); */\nvoid f_b(void);\n"
                        "const char* f_c(cdx_stream_t s);  // int f_not(int)\nsize_t f_d(const cdx_hand *h, int n);",
                        "f_", ";")
    assert protos == {"f_a": ("int", ["cdx_chain*", "double*"]), "f_b": ("void", []),
                      "f_c": ("char*", ["cdx_stream_t"]), "f_d": ("size_t", ["cdx_hand*", "int"])}
    from compliancedex_amd._native import CdxChain
    good = {"f_a": (C.c_int, [C.POINTER(CdxChain), C.c_void_p]), "f_b": (None, []),
            "f_c": (C.c_char_p, [C.c_void_p]), "f_d": (C.c_size_t, [C.c_void_p, C.c_int32])}
    assert abi_mismatches(protos, good) == []
    bad = {"f_a": (C.c_int, [C.POINTER(CdxChain), C.c_int64]), "f_b": (C.c_int, []),
           "f_c": (C.c_char_p, [C.c_void_p]), "f_d": (C.c_size_t, [C.POINTER(CdxChain), C.c_int32]),
           "f_e": (None, [])}
    assert abi_mismatches(protos, bad) == [("f_e", "undeclared"), ("f_a", "arg 1"), ("f_b", "return"),
                                           ("f_d", "arg 0")]


def test_bindings_live_in_their_two_modules():
    """Outside _native.py, _host.py and tests/_sdf_oracle.py (another library) no Python file of tests/, tools/ or the
    package opens a library itself or assigns a signature: a cdxh_* function is bound by its line in _host._SIGS.
    (The cdx_diag_* symbols of the timing-only diagnostic builds are bound where their tool loads such a build.)"""
    skip = {os.path.join("compliancedex_amd", "_native.py"), os.path.join("compliancedex_amd", "_host.py"),
            os.path.join("tests", "_sdf_oracle.py")}
    found = []
    for top in ("tests", "tools", "compliancedex_amd"):
        for root, _, files in os.walk(os.path.join(REPO, top)):
            for name in files:
                path = os.path.relpath(os.path.join(root, name), REPO)
                if not name.endswith(".py") or path in skip:
                    continue
                for i, line in enumerate(open(os.path.join(REPO, path), encoding="utf-8"), 1):
                    sig = re.search(r"(\w+)\.(argtypes|restype)\s*=[^=]", line)
                    if re.search(r"CDLL\(", line) or (sig and not sig.group(1).startswith("cdx_diag_")):
                        found.append(f"{path}:{i}: {line.strip()}")
    assert found == []


def test_library_exports_every_declared_symbol():
    from compliancedex_amd import _native
    lib = _native.load()  # also checks struct sizes against the library
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert lib.cdx_version().startswith(b"compliancedex_amd")


def test_native_sources_read_only_the_two_oracle_switches():
    """No variable in a user's environment changes what the native library computes or how it schedules it: over
    every file of csrc/, the only reads of the environment are the getenv calls for CDX_KABSCH_AHEAD and CDX_VAR_LATE
    (the two bit-parity oracle switches of tests/test_screen.py), each naming its variable by a string literal, and
    no other function whose name holds "env" (a gated or secure reader, a wrapper, setenv / putenv) is defined or
    called.  (tests/test_screen.py::test_env_switches_cannot_disable_the_repair runs the closure with the retired
    screen switches set on the GPU.)"""
    from compliancedex_amd.build import CSRC
    read, calls = set(), 0
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name), encoding="utf-8").read()
        assert set(re.findall(r"\b(\w*env\w*)\s*\(", text, re.I)) <= {"getenv"}, name
        assert "environ" not in text, name
        calls += len(re.findall(r"\bgetenv\b", text))
        read |= set(re.findall(r'\bgetenv\s*\(\s*"([^"]*)"\s*\)', text))
    assert read == {"CDX_KABSCH_AHEAD", "CDX_VAR_LATE"}
    assert calls == 2  # (no call with a computed name, no second reader of either, no mention elsewhere)


def test_build_macros_are_the_documented_ones():
    """The product is a plain compile of csrc/ (no -D), and the only CDX_* macros a preprocessor conditional there
    tests are the ones DESIGN.md §2a lists under "Build macros": the timing-only diagnostic builds.  A
    measured-and-lost variant kept behind a new macro fails here."""
    from compliancedex_amd.build import CSRC, DEFAULT_DEFINES
    assert tuple(DEFAULT_DEFINES) == ()
    used = set()
    for name in os.listdir(CSRC):
        for line in open(os.path.join(CSRC, name), encoding="utf-8"):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                used |= set(re.findall(r"\bCDX_[A-Z0-9_]+", line))
    design = open(os.path.join(REPO, "DESIGN.md"), encoding="utf-8").read()
    section = design.split("### Build macros", 1)[1].split("\n#", 1)[0]
    documented = set()
    for row in section.splitlines():
        if row.startswith("| `CDX_"):
            documented |= set(re.findall(r"`(CDX_[A-Z0-9_]+)`", row.split("|")[1]))
    assert used == documented, (sorted(used - documented), sorted(documented - used))


def test_bad_arguments_are_rejected_without_launch():
    import ctypes
    from compliancedex_amd import _native as N
    lib = N.load()
    g = N.CdxGpis()
    assert lib.cdx_gpis_mean(g, None, 10, None, None, None, None) == -1
    g.kernel = 7
    g.X1 = g.alpha = 1
    g.N, g.N_pad = 1, 64
    assert lib.cdx_gpis_mean(g, None, 10, None, None, None, None) == -2
    c = N.CdxChain()
    assert lib.cdx_fk_forward(c, None, 1, None, None, None) == -3
    assert lib.cdx_sdf_forward(None, 5, None, 0, None, None, None, None, None, None) == -1
    assert lib.cdx_sdf_query(None, None, 0, None, 5, None, None, None, None, None, None, 0, 0, None) == -1
    assert lib.cdx_sdf_query_workspace(0) == 0 and lib.cdx_sdf_mesh_bytes(0) == 0
    assert lib.cdx_sdf_mesh_prepare(None, 10, None, None) == -1
    assert lib.cdx_sdf_query_order(None, 5, None, 0, None) == -1 and lib.cdx_sdf_query_order(None, -1, None, 0, None) == -1
    assert lib.cdx_sdf_query_batch(5, None, None, 0, None) == -1 and lib.cdx_sdf_query_batch(1, None, None, 0, None) == -1
    q = N.CdxSdfBatchQuery()
    q.P, q.F, q.flags = 10, 4, N.SDF_REUSE_ORDER  # (not marked culled)
    assert lib.cdx_sdf_query_batch(1, ctypes.cast(ctypes.pointer(q), ctypes.c_void_p), None, 0, None) == -1
    # the launch schedule: 4 header words, then a duration and an order slot per 64-point group
    Ps = (ctypes.c_int64 * 3)(65536, 65536, 100)
    assert lib.cdx_sdf_batch_schedule_bytes(3, Ps) == 4 * (4 + 2 * (1024 + 1024 + 2))
    assert lib.cdx_sdf_batch_schedule_bytes(5, Ps) == 0 and lib.cdx_sdf_batch_schedule_bytes(1, None) == 0
    cfg, buf = N.CdxKinOpt(), N.CdxKinOptBuffers()
    cfg.rule = 2
    assert lib.cdx_kin_step(None, cfg, buf, 4, 4, 0, 0, None) == -1  # unknown rule
    cfg.rule = 0
    assert lib.cdx_kin_step(None, cfg, buf, 4, 4, 0, 0, None) == -1  # Adam (Kin) without a chain
    cfg.rule = 1
    assert lib.cdx_kin_step(None, cfg, buf, 4, 4, 0, 0, None) == -1  # null buffers
    prm = N.CdxKinParams()
    prm.fe.n_tips = 4
    assert lib.cdx_kin_iteration(None, None, cfg, buf, 4, 4, *[None] * 10, 0, 0, None) == -1  # no params
    cfg.rule = 0
    assert lib.cdx_kin_iteration(None, prm, cfg, buf, 4, 4, *[None] * 10, 0, 0, None) == -1  # Kin without a chain
    assert lib.cdx_kin_iteration(c, prm, cfg, buf, 4, 3, *[None] * 10, 0, 0, None) == -1  # tip count mismatch
    # the FK-walk cache: one block of (12 + 6·16 + 8 + 4) slots × 64 lanes of floats per 64-lane workgroup (four lanes
    # a candidate), none for other fingertip counts or no candidates
    assert lib.cdx_kin_fk_state_bytes(16384, 4) == 1024 * 120 * 64 * 4
    assert lib.cdx_kin_fk_state_bytes(3000, 4) == 188 * 120 * 64 * 4
    assert lib.cdx_kin_fk_state_bytes(3000, 3) == 0 and lib.cdx_kin_fk_state_bytes(0, 4) == 0
    p = N.CdxProblem()
    assert lib.cdx_closure_workspace(p, 10) == 0
    assert lib.cdx_closure(p, 10, *([None] * 6), ctypes.c_uint64(0), *([None] * 11)) == -1


def test_product_refuses_cpu_tensors():
    import pytest
    import torch
    from compliancedex_amd import GPIS
    g = GPIS(0.08, 1.0)
    g.load_state_data("banana_state", device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.pred(torch.zeros(4, 3, dtype=torch.float64))


def test_batch_schedule_host_logic():
    """torchsdf.BatchSchedule (host side of cdx_sdf_query_batch's schedule): sized by cdx_sdf_batch_schedule_bytes,
    zeroed when (re)allocated, the order recomputed on every `every`-th launch and whenever the group count changes."""
    import torch
    from compliancedex_amd.torchsdf import BatchSchedule
    dev = torch.device("cpu")
    sch = BatchSchedule(every=4)
    buf = sch.get([65536, 65536, 100], dev)
    assert buf.numel() == 4 * (4 + 2 * (1024 + 1024 + 2)) and int(buf.sum()) == 0
    keeps = [sch.keep_order() for _ in range(9)]
    assert keeps == [False, True, True, True, False, True, True, True, False]
    sch.get([6000, 6000, 3000], dev)  # fewer groups: the same buffer, the order recomputed next
    assert sch.buf is buf and sch.keep_order() is False and sch.keep_order() is True
    big = sch.get([1 << 20], dev)  # more groups than the buffer holds: a new, zeroed buffer
    assert big is not buf and big.numel() == 4 * (4 + 2 * 16384) and sch.keep_order() is False
