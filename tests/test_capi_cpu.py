"""CPU: the C-ABI library loads and exports every symbol include/riggs_hip.h declares; host-side
logic that needs no GPU."""
import os
import re

import pytest
import torch

from riggs_amd import _lib


def _header_functions():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "riggs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(riggs_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    declared = _header_functions()
    assert len(declared) >= 18
    L = _lib.lib()  # loads without a GPU; argtypes set for every symbol
    for name in declared:
        assert hasattr(L, name), "symbol %s declared in include/riggs_hip.h but not exported" % name
    assert sorted(_lib.exported_symbols()) == declared
    assert L.riggs_version() >= 100


# ---- the binding is read from the header (riggs_amd/_abi.py): here the COMPILER reads the same header and has to agree
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
_STRUCT_NAMES = {"RasterCfg": "riggs_raster_cfg", "Frame": "riggs_frame", "FrameGrads": "riggs_frame_grads",
                 "MlpEpilogue": "riggs_mlp_epilogue", "GateStruct": "riggs_gate", "NodeMlp": "riggs_node_mlp",
                 "NodeMlpGrads": "riggs_node_mlp_grads", "ViewerProjection": "riggs_viewer_projection", "ViewerFrame": "riggs_viewer_frame"}
_CHECKS = """#include <tuple>
#include <type_traits>
#include "riggs_hip.h"
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
  using ret = R;
  static constexpr int arity = sizeof...(A);
  template <int i> using arg = std::tuple_element_t<i, std::tuple<A...>>;
};
template <class T> constexpr bool ptr() { return std::is_pointer<T>::value; }
template <class T, class S> constexpr bool ptr_to() { return ptr<T>() && std::is_same<std::remove_cv_t<std::remove_pointer_t<T>>, S>::value; }
template <class T, int n> constexpr bool sint() { return std::is_integral<T>::value && std::is_signed<T>::value && sizeof(T) == n; }
template <class T, int n> constexpr bool uint() { return std::is_integral<T>::value && std::is_unsigned<T>::value && sizeof(T) == n; }
template <class T> constexpr bool flt() { return std::is_same<T, float>::value; }
template <class T> constexpr bool dbl() { return std::is_same<T, double>::value; }
"""


def _kind(t, of):
    """The C++ predicate a ctypes class stands for: pointer (to a struct / to char), float, double, (un)signed integer by size."""
    import ctypes as C
    if t is C.c_void_p:
        return "ptr<%s>()" % of
    if t is C.c_char_p:
        return "ptr_to<%s, char>()" % of
    if hasattr(t, "contents"):  # POINTER(Structure)
        return "ptr_to<%s, %s>()" % (of, t._type_.__name__)
    if t in (C.c_float, C.c_double):
        return ("flt<%s>()" if t is C.c_float else "dbl<%s>()") % of
    assert t._type_ in "iIlLqQ", t
    return "%s<%s, %d>()" % ("sint" if t._type_ in "ilq" else "uint", of, C.sizeof(t))


def _signature_checks(table):
    lines = [_CHECKS]
    for k, (name, (res, args)) in enumerate(sorted(table.items())):
        lines.append("using F%d = sig<decltype(&%s)>;" % (k, name))
        lines.append('static_assert(F%d::arity == %d, "%s: arity");' % (k, len(args), name))
        lines.append('static_assert(%s, "%s: return");' % (_kind(res, "F%d::ret" % k), name))
        lines += ['static_assert(%s, "%s[%d]");' % (_kind(a, "F%d::arg<%d>" % (k, i)), name, i) for i, a in enumerate(args)]
    return "\n".join(lines) + "\n"


def _gxx(tmp_path, name, source, *flags):
    import subprocess
    path = tmp_path / name
    path.write_text(source)
    return subprocess.run(["g++", "-std=c++17", "-I", _INCLUDE, str(path)] + list(flags), capture_output=True, text=True)


def test_binding_matches_what_the_compiler_sees_in_the_header(tmp_path):
    """Every function of the derived table as static_asserts on decltype(&riggs_x): arity, the return kind and per argument
    pointer (to the named struct, to char) / float / double / signed or unsigned integer of 4 or 8 bytes.  The compiler is the
    oracle, not the parser.  Two deliberately wrong tables must fail to compile: the check can fail."""
    import ctypes as C
    table = dict(_lib._SIGS)
    assert len(table) == len(_header_functions())
    ok = _gxx(tmp_path, "sigs.cpp", _signature_checks(table), "-fsyntax-only")
    assert ok.returncode == 0, ok.stderr[-4000:]
    res, args = table["riggs_lbs_forward"]
    at = max(i for i, a in enumerate(args) if a is C.c_void_p)
    short = dict(table, riggs_lbs_forward=(res, args[:at] + args[at + 1:]))            # one pointer fewer
    bad = _gxx(tmp_path, "short.cpp", _signature_checks(short), "-fsyntax-only")
    assert bad.returncode != 0 and "riggs_lbs_forward: arity" in bad.stderr
    res, args = table["riggs_adam_step"]
    at = args.index(C.c_double)
    narrow = dict(table, riggs_adam_step=(res, args[:at] + [C.c_float] + args[at + 1:]))  # a float where the header has double
    bad = _gxx(tmp_path, "narrow.cpp", _signature_checks(narrow), "-fsyntax-only")
    assert bad.returncode != 0 and "riggs_adam_step[%d]" % at in bad.stderr


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    """sizeof / offsetof / field size of the header's nine structs as the compiler lays them out against the derived
    ctypes.Structure classes, and the value of every enumerator and #define against the derived constants."""
    import ctypes as C
    import subprocess
    from riggs_amd import _abi, viewer
    assert {n: getattr(_lib, p).__name__ for p, n in _STRUCT_NAMES.items()} == {n: n for n in _abi.STRUCTS}
    body = []
    for name, cls in _abi.STRUCTS.items():
        body.append('  printf("S %s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            body.append('  printf("F %s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
    body += ['  printf("K %s %%lld\\n", (long long)%s);' % (k, k) for k in _abi.CONSTANTS]
    src = '#include <cstddef>\n#include <cstdio>\n#include "riggs_hip.h"\nint main() {\n%s\n  return 0;\n}\n' % "\n".join(body)
    exe = tmp_path / "layout"
    built = _gxx(tmp_path, "layout.cpp", src, "-o", str(exe))
    assert built.returncode == 0, built.stderr[-4000:]
    seen = [l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    mine = [["S", n, str(C.sizeof(c))] for n, c in _abi.STRUCTS.items()]
    mine += [["F", "%s.%s" % (n, f), str(getattr(c, f).offset), str(getattr(c, f).size)] for n, c in _abi.STRUCTS.items() for f, _ in c._fields_]
    mine += [["K", k, str(v)] for k, v in _abi.CONSTANTS.items()]
    assert sorted(seen) == sorted(mine)
    assert len(_abi.STRUCTS) == 9 and sum(len(c._fields_) for c in _abi.STRUCTS.values()) == 160
    # ... and the short names the package uses are those constants
    K = _abi.CONSTANTS
    assert (_lib.GEOM_XYD, _lib.GEOM_DEPTH_ORDER, _lib.GEOM_NFIELDS) == (K["RIGGS_GEOM_XYD"], K["RIGGS_GEOM_DEPTH_ORDER"], K["RIGGS_GEOM_NFIELDS_"])
    assert (_lib.IMG_FWD_CTR, _lib.IMG_NFIELDS, _lib.BIN_WALK_HIST, _lib.BIN_NFIELDS) == \
        (K["RIGGS_IMG_FWD_CTR"], K["RIGGS_IMG_NFIELDS_"], K["RIGGS_BIN_WALK_HIST"], K["RIGGS_BIN_NFIELDS_"])
    for short in ("PRIM_WORDS", "MAX_TABLES", "SEGMENT", "DISC", "SQUARE", "RULE_EDITOR", "RULE_RENDER_RIG", "LAYOUT_SKELETON",
                  "LAYOUT_SQUARES", "LAYOUT_POLYLINES", "BLEND_ALPHA", "BLEND_MASK", "MODE_IMAGE", "MODE_DEPTH", "MODE_ALPHA", "MODE_NORMAL"):
        assert getattr(viewer, short) == K["RIGGS_VIEWER_" + short], short


def test_untyped_out_pointers_still_take_byref_and_arrays():
    """The host out-pointers the header types as plain pointers (int32_t*, size_t*) are c_void_p in the derived table; they take
    byref(...) and ctypes arrays as before.  The offsets are those of the library before the binding was derived (N = 1000,
    H = W = 64, capacity 4096)."""
    import ctypes as C
    L = _lib.lib()
    go, io, bo = (C.c_size_t * _lib.GEOM_NFIELDS)(), (C.c_size_t * _lib.IMG_NFIELDS)(), (C.c_size_t * _lib.BIN_NFIELDS)()
    assert L.riggs_raster_geom_layout(1000, go) == 0 and list(go) == [0, 16128, 32256, 48384, 72448, 73472, 77568, 93952]
    assert L.riggs_raster_image_layout(64, 64, io) == 0 and list(io) == [0, 16384, 98304, 99328]
    assert L.riggs_raster_binning_layout(4096, 1000, 64, 64, bo) == 0 and list(bo) == [0, 16384, 457984]
    offset, size = C.c_size_t(), C.c_size_t()
    assert L.riggs_raster_backward_workspace_rows(1000, C.byref(offset), C.byref(size)) == 0 and (offset.value, size.value) == (48128, 128)
    before, v = _lib.get_option("fwd_wide_min"), C.c_int32(-1)
    try:
        _lib.set_option("fwd_wide_min", 5000)
        assert L.riggs_get_option(b"fwd_wide_min", C.byref(v)) == 0 and v.value == 5000
    finally:
        _lib.set_option("fwd_wide_min", before)
    assert _lib.get_option("fwd_wide_min") == before
    assert L.riggs_get_option(b"no_such_option", C.byref(v)) != 0
    # how each option takes a value: (set, stored) pairs; the last pair puts the default back
    takes = {"fwd_wide_tiles": ((70000, 65535), (0, 0), (-1, 256)), "fwd_wide_min": ((100, 256), (0, 256), (-7, 4096)),
             "fwd_hist_view_tol": ((0, 0), (10 ** 6, 10 ** 6), (-1, 20)), "color_side_jobs": ((0, 0), (5, 1), (-5, 1)),
             "pose_mlp_layered": ((5, 1), (-5, 1), (0, 0)), "bin_grouped": ((1, 1), (0, 0), (-1, -1)),
             "preprocess_bwd_lean": ((1, 1), (0, 0), (-1, -1)), "lbs_scalar": ((1, 1), (-1, -1), (0, 0))}
    try:
        for name, pairs in takes.items():
            default = _lib.get_option(name)
            assert default == pairs[-1][1], name
            for given, stored in pairs:
                assert L.riggs_set_option(name.encode(), given) == 0 and _lib.get_option(name) == stored, (name, given)
        # the three with a closed set of values refuse anything else with rc 2, say which values they take, and keep what they had
        for name, accepts in (("bin_grouped", b"bin_grouped takes -1 (by size), 0 or 1"),
                              ("preprocess_bwd_lean", b"preprocess_bwd_lean takes -1 (with cfg.sparse_zero), 0 or 1"),
                              ("lbs_scalar", b"lbs_scalar takes -1 (never), 0 (by size) or 1 (always)")):
            for bad in (-2, 2):
                assert L.riggs_set_option(name.encode(), bad) == 2 and accepts in L.riggs_last_error(), (name, bad)
            assert _lib.get_option(name) == takes[name][-1][1]
        assert L.riggs_set_option(b"no_such_option", 1) == 2 and b"unknown option 'no_such_option'" in L.riggs_last_error()
    finally:
        for name, pairs in takes.items():
            _lib.set_option(name, pairs[-1][0])
    # the option that selected the control-node backward's first design left with that design: an unknown name now
    assert L.riggs_set_option(b"cnode_bwd_atomics", 1) != 0 and L.riggs_get_option(b"cnode_bwd_atomics", C.byref(v)) != 0


def test_library_and_header_versions_agree(monkeypatch):
    from riggs_amd import _abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(_INCLUDE, "riggs_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+riggs_version\s*\(\s*void\s*\)", hdr)
    assert _lib.lib().riggs_version() == _lib.ABI_VERSION == _abi.CONSTANTS["RIGGS_ABI_VERSION"]
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(_lib.RiggsHipError, match="rebuild"):
        _lib.lib()


@pytest.mark.parametrize("after, added", [
    ("int riggs_prof_reset(void);", "int riggs_walk(int (*visit)(int32_t), riggs_stream stream);"),   # a function pointer
    ("int riggs_prof_reset(void);", "int riggs_take(riggs_unknown by_value);"),                        # a type nobody declared
    ("int riggs_prof_reset(void);", "enum { RIGGS_SHIFTED = 1 << 3 };"),                               # an expression
])
def test_a_declaration_the_reader_cannot_read_raises_with_its_line(tmp_path, monkeypatch, after, added):
    """Nothing is skipped silently: a header that leaves the style riggs_amd/_abi.py reads fails at load, naming the line."""
    from riggs_amd import _abi
    text = open(_abi.HEADER).read().replace(after, after + "\n" + added)
    (tmp_path / "riggs_hip.h").write_text(text)
    for table in ("FUNCTIONS", "STRUCTS", "CONSTANTS", "_TYPES"):   # (the reader fills these: fresh ones, the real ones stay)
        monkeypatch.setattr(_abi, table, dict(getattr(_abi, table)))
    monkeypatch.setattr(_abi, "HEADER", str(tmp_path / "riggs_hip.h"))
    line = text[:text.index(added)].count("\n") + 1
    with pytest.raises(_abi.HeaderError, match=r"riggs_hip\.h:%d: cannot read" % line):
        _abi._read()


def test_stale_extension_is_refused(monkeypatch):
    """An extension built against another RIGGS_ABI_VERSION than the library's is not used: the ctypes nodes run."""
    from riggs_amd import _torch_ext as TX
    if not os.path.exists(TX.PATH):
        pytest.skip("lib/libriggs_torch.so is not built")
    L = _lib.lib()
    monkeypatch.setitem(TX._state, "loaded", None)
    assert TX.available()
    monkeypatch.setitem(TX._state, "loaded", None)
    monkeypatch.setattr(L, "riggs_version", lambda: _lib.ABI_VERSION + 1)
    assert not TX.available() and not TX.active()


def test_product_path_refuses_cpu_tensors():
    from riggs_amd.rasterizer import GaussianRasterizer, GaussianRasterizationSettings
    st = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3,
                                       torch.zeros(3), False, False)
    r = GaussianRasterizer(st)
    with pytest.raises(_lib.RiggsHipError, match="CUDA"):
        r(means3D=torch.zeros(4, 3), means2D=torch.zeros(4, 3), opacities=torch.zeros(4, 1), shs=torch.zeros(4, 16, 3),
          scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=torch.zeros(4, 3), means2D=None, opacities=torch.zeros(4, 1), scales=torch.ones(4, 3),
          rotations=torch.ones(4, 4))


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", "/nonexistent/libriggs_hip.so")
    with pytest.raises(_lib.RiggsHipError, match="no fallback"):
        _lib.lib()


def test_skeleton_host_logic_cpu():
    from riggs_amd.skeleton import SkeletonWarp
    joints = torch.randn(5, 3)
    sw = SkeletonWarp(joints=joints, parent_indices=torch.tensor([-1, 0, 1, 1, 3]), K=-1, hyper_dim=8,
                      use_skinning_weight_mlp=False, use_template_offsets=False)
    assert sw.nodes.shape == (5, 11) and not sw.nodes.requires_grad
    assert sw.expand_time(torch.tensor([0.5])).shape == (5, 1)
    info = sw.get_pose_info(sw.expand_time(torch.tensor([0.5])))
    assert info["local_rotation"].shape == (5, 4) and info["global_trans"].shape == (3,)
    names = [g["name"] for g in sw.trainable_parameters()]
    assert names == ["nodes", "pose"]
    keys = set(sw.state_dict().keys())
    assert {"nodes", "_node_radius", "control_nodes", "pose_net.rotation_predictor.weight"} <= keys
    with pytest.raises(ValueError):
        bad = SkeletonWarp(joints=joints, parent_indices=torch.tensor([-1, 2, 1, 1, 3]), K=-1,
                           use_skinning_weight_mlp=False, use_template_offsets=False)
        bad._parents_dev(torch.device("cpu"))


def test_argument_validation_of_the_next_row_entries_needs_no_gpu():
    """Bad sizes / NULL buffers are rejected with a message before any HIP call (no compute, no GPU)."""
    L = _lib.lib()
    N = None
    # control nodes: K > 8, hyper > 11, K > M
    for (n, m, k, hyper) in ((10, 32, 9, 0), (10, 32, 3, 12), (10, 2, 3, 0)):
        rc = L.riggs_cnode_forward(n, m, k, hyper, hyper, 3 + hyper, 0, *([N] * 17))
        assert rc != 0 and L.riggs_last_error()
    assert L.riggs_cnode_forward(10, 32, 3, 0, 0, 3, 1, *([N] * 17)) != 0            # local_frame without local_rotation
    assert b"local_rotation" in L.riggs_last_error()
    assert L.riggs_cnode_backward_workspace_floats(1000, 64, 3, 8) >= 33 * 3000
    assert L.riggs_cnode_backward_workspace_floats(10, 64, 3, 8) == 1127  # 33 N K + one list block's M + M + 1 + 8
    # skeleton projection loss: one joint, empty sample / pixel sets, too many samples per bone
    for (j, s, m) in ((1, 4, 4), (5, 0, 4), (5, 4, 0), (5, 4096, 4)):
        rc = L.riggs_skeleton_projection_forward(j, s, m, N, N, N, N, 1.0, 1.0, 0.0, 0.0, N, N, N, N, N, N)
        assert rc != 0 and L.riggs_last_error()
    assert L.riggs_skeleton_projection_state_floats(24, 41, 1500) == 2 * 41 * 23 + 2 * 1500 + 6 * 23
    # fused MLP heads: the cotangent without a g_eff is g alone (dummy non-NULL pointers: refused before any launch) ...
    P = 4096
    for g_rows, sig, l2_out, l2_coef in ((P, N, N, N), (N, P, N, N), (N, N, P, P)):
        rc = L.riggs_mlp_cotangent(8, 3, P, g_rows, N, sig, l2_out, l2_coef, N, P, P, P, N, N)
        assert rc != 0 and b"g_eff" in L.riggs_last_error()
    assert L.riggs_mlp_cotangent(8, 3, N, N, N, N, N, N, N, P, P, P, N, N) != 0 and b"g_eff" in L.riggs_last_error()  # (nor without g)
    # ... and the weight gradients of a constant tail need the tail
    rc = L.riggs_mlp_wgrad(8, 27, 96, N, 3, 8, 4, *([P] * 6), 1 << 20, *([P] * 4), N, 1, N)
    assert rc != 0 and b"tail" in L.riggs_last_error()


def test_integration_stub_matches_the_header_struct():
    """INTEGRATION.md's ctypes stub of riggs_raster_cfg, the struct in include/riggs_hip.h and riggs_amd._lib.RasterCfg
    list the same fields in the same order (a binding written from a stale stub makes the library read past the struct)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    stub = doc[doc.index("class RasterCfg(C.Structure)"):]
    stub = stub[:stub.index("def rasterize")]
    stub_fields = re.findall(r'\("([a-z_0-9A-Z]+)",\s*C\.(c_[a-z0-9_]+)\)', stub)
    import ctypes as C
    canon = lambda name: getattr(C, name).__name__            # (c_int32 is an alias of c_int on this ABI)
    mine = [(n, t.__name__) for n, t in _lib.RasterCfg._fields_]
    assert [(n, canon(t)) for n, t in stub_fields] == mine
    hdr = open(os.path.join(root, "include", "riggs_hip.h")).read()
    body = hdr[hdr.index("typedef struct riggs_raster_cfg"):hdr.index("} riggs_raster_cfg;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    hdr_fields = re.findall(r"\b(?:const\s+)?(int32_t|float)\s*(\*?)\s*([a-zA-Z_0-9]+)\s*;", body)
    ctype = {("int32_t", ""): "c_int32", ("float", ""): "c_float", ("float", "*"): "c_void_p"}
    assert [(n, canon(ctype[(t, p)])) for t, p, n in hdr_fields] == mine
    # the stub's constructor call passes one value per field
    call = stub_fields and doc[doc.index("cfg = RasterCfg("):]
    call = call[:call.index("\n    u8 =")]
    depth, n_args = 0, 1
    for ch in call[call.index("(") + 1:call.rindex(")")]:
        depth += ch in "([" 
        depth -= ch in ")]"
        n_args += (ch == "," and depth == 0)
    assert n_args == len(mine)


def test_pose_mlp_sync_buffer_is_as_large_as_the_library_wants():
    """PoseMLP restates riggs_pose_mlp_sync_bytes for its persistent hand-off state (built on CPU-only hosts too); a buffer
    that is too small silently falls back to a per-launch private state (no sticky status word)."""
    from riggs_amd import _lib as L
    from riggs_amd.skeleton import PoseMLP
    for joints, depth, width in ((24, 8, 256), (64, 8, 256), (6, 3, 32), (12, 12, 128)):
        net = PoseMLP(1, joints * 4, hidden_dimensions=width, depth=depth)
        assert net._hip_sync.numel() * 4 >= L.lib().riggs_pose_mlp_sync_bytes(depth, width)
        assert int(L.lib().riggs_pose_mlp_status_word(depth, width)) + 1 < net._hip_sync.numel()


def test_torch_extension_loads_and_registers_its_ops():
    """lib/libriggs_torch.so (riggs_amd/csrc_torch/riggs_torch.cpp; built by __graft_entry__.build()): loads next to libriggs_hip.so
    without a GPU, speaks the library's ABI version and registers the two nodes' ops (no compute call here)."""
    import torch
    from riggs_amd import _lib as L
    from riggs_amd import _torch_ext as TX
    from riggs_amd import build as B
    B.build_torch()
    assert TX.available()
    assert int(torch.ops.riggs.abi_version()) == int(L.lib().riggs_version())
    for name in ("pose_deform", "glue_raster"):
        assert hasattr(torch.ops.riggs, name)
    sch = str(torch.ops.riggs.glue_raster.default._schema)
    assert "Tensor? d_xyz" in sch or "Tensor?" in sch
