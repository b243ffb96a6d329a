"""-m "not gpu": the C-ABI library builds for gfx950, loads, and exports every symbol that
include/seedvr2_hip.h declares (no compute calls without a GPU); the product refuses to run without it."""
import ctypes
import os
import re
import shutil

import pytest
import torch

from conftest import sub, ROOT

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def _declared():
    src = open(os.path.join(ROOT, "include", "seedvr2_hip.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(svr_\w+)\s*\(", src, flags=re.M)))


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_library_builds_loads_and_exports_header_symbols():
    hip_lib = sub("hip_lib")
    path = hip_lib.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    declared = _declared()
    assert len(declared) >= 17
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in seedvr2_hip.h but not exported"
    assert sorted(hip_lib.SYMBOLS) == declared, "ctypes table and header disagree"
    lib.svr_abi_version.restype = ctypes.c_int
    assert lib.svr_abi_version() == hip_lib.ABI_VERSION == 9
    assert hip_lib.lib().svr_abi_version() == 9
    # the binary carries the content hash of the sources it was compiled from; the loader refuses any other
    assert hip_lib.built_id() == hip_lib.source_id() and not hip_lib.needs_build()


def test_struct_layout_matches_header():
    hip_lib = sub("hip_lib")
    # svr_conv_geom: 18 int32 + 2 pointers; svr_pixel_shuffle: 7 int32
    assert ctypes.sizeof(hip_lib.ConvGeom) == 18 * 4 + 2 * 8
    assert ctypes.sizeof(hip_lib.PixelShuffle) == 7 * 4
    # svr_phase_scatter: 4 int32 + pointer + 2 int32 + 3 x 4 pointers (ABI v6: the quad launch)
    assert ctypes.sizeof(hip_lib.PhaseScatter) == 4 * 4 + 8 + 2 * 4 + 12 * 8 and hip_lib.GemmArgs.phase.offset % 8 == 0
    assert hip_lib.GemmArgs.conv.offset % 8 == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a GPU-less host")
def test_product_fails_loudly_without_gpu():
    ops, hip_lib = sub("ops"), sub("hip_lib")
    with pytest.raises(hip_lib.HipLibraryError):
        ops.HipOps("cpu")
    with pytest.raises(Exception):
        ops.HipOps("cuda:0")


def test_svr_options_environment_reaches_the_library():
    """SVR_OPTIONS="key=value,..." is applied through svr_set_option when the library is loaded (the measurement scripts'
    only channel: round 2 found getenv() calls inside static-initialiser lambdas of the .hip sources reading the WRONG
    variable, which silently turned three A/B runs into A/A runs); an unknown key or a malformed item is an error."""
    import subprocess
    import sys
    from conftest import ROOT
    code = (
        "import ctypes, importlib, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "m = importlib.import_module('comfyui-seedvr2_videoupscaler_amd.hip_lib')\n"
        "L = m.lib()\n"
        "print(ctypes.c_int.in_dll(L, '_ZN3svr11g_conv_rowsE').value, ctypes.c_int.in_dll(L, '_ZN3svr10g_gemm_epiE').value,"
        " ctypes.c_int.in_dll(L, '_ZN3svr14g_conv_lds_dbgE').value)\n")
    env = dict(os.environ, SVR_OPTIONS="conv_rows=8, gemm_epi=2,conv_lds=100000")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["8", "2", "100000"]
    env.pop("SVR_OPTIONS")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[1:] == ["0", "0"], (r.stdout, r.stderr)      # defaults
    for bad in ("no_such_key=1", "conv_rows"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(env, SVR_OPTIONS=bad), capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "SVR_OPTIONS" in r.stderr


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_loader_refuses_a_binary_built_from_other_sources(tmp_path, monkeypatch):
    """svr_build_id() is the content hash of the sources the binary was compiled from: after any source edit (here: one more
    header in the source list) the library counts as stale -- build() would recompile, lib() refuses to load it."""
    hip_lib = sub("hip_lib")
    hip_lib.build()
    extra = tmp_path / "svr_extra.h"
    extra.write_text("// an edit\n")
    real = hip_lib.sources
    monkeypatch.setattr(hip_lib, "sources", lambda: real() + [str(extra)])
    assert hip_lib.needs_build()
    monkeypatch.setattr(hip_lib, "_lib", None)
    with pytest.raises(hip_lib.HipLibraryError, match="other sources"):
        hip_lib.lib()


def test_build_id_covers_the_compile_configuration(monkeypatch):
    """A measurement build (-DSVR_ABLATIONS: kernel variants that give garbage on purpose) compiled from the same sources must not
    pass for the product build: the id hashes flags and defines too."""
    hip_lib = sub("hip_lib")
    monkeypatch.delenv("SVR_BUILD_ABLATIONS", raising=False)
    product = hip_lib.source_id()
    monkeypatch.setenv("SVR_BUILD_ABLATIONS", "1")
    assert hip_lib.source_id() != product
    monkeypatch.delenv("SVR_BUILD_ABLATIONS")
    monkeypatch.setattr(hip_lib, "HIPCC_FLAGS", hip_lib.HIPCC_FLAGS + ["-O1"])
    assert hip_lib.source_id() != product


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_kernel_classifier_on_the_launches_a_vae_tile_issues():
    """bench.py attributes launch times to kernels with svr_gemm_kernel_class() -- the routing function the launch itself uses
    (csrc/svr_gemm.hip gemm_route), so the two cannot disagree.  Here the engine's host code runs over shape-only tensors
    (tools/shape_census.py) and every gemm call of one 1024-px tile, encode and decode, is classified by the library:
    stride-1 3x3 convs -> the LDS-halo kernel (the `roofline` kernel) and NOTHING else lands in that class."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shape_census
    sub("hip_lib").build()
    config, weights, vae = sub("config"), sub("weights"), sub("vae")
    cfg = config.VAE_V3
    eng_ops = shape_census.MetaOps(classify=True)
    eng = vae.VideoVAEEngine(cfg, weights.synth_vae_state_dict(cfg, device="meta"), eng_ops)
    eng.decode_clip(torch.empty(3, 128, 128, cfg.latent_channels, dtype=torch.bfloat16, device="meta"))
    eng.encode_clip(torch.empty(9, 1024, 1024, 4, dtype=torch.bfloat16, device="meta"))
    seen = {}
    for cls, g, M, N, K in eng_ops.launches:
        assert cls != "invalid"
        seen[cls] = seen.get(cls, 0) + 1
        if g is None:
            assert cls in ("gemm", "gemm_persistent")
            continue
        same = tuple(g.stride) == (1, 1, 1) and g.Ho == g.H and g.Wo == g.W
        if cls == "conv_halo":
            assert g.k[1:] == (3, 3) and same and g.Cin % 64 == 0 and N % 128 == 0
        elif cls == "conv_subpixel":
            assert g.k[1:] == (2, 2) and same
        elif cls == "conv_thin_in":
            assert g.Cin == 4 and N == 128
        elif cls == "conv_thinout":
            assert g.k[1:] == (3, 3) and same and N <= 32
        else:
            assert cls == "conv_generic" and (not same or g.k[1:] == (1, 1) or g.Cin % 64 != 0), (g, N)
        if g.k[1:] == (3, 3) and same and g.Cin % 64 == 0 and N % 128 == 0:
            assert cls == "conv_halo"
    assert {"conv_halo", "conv_subpixel", "conv_thin_in", "conv_thinout", "conv_generic", "gemm"} <= set(seen), seen
    # the NaDiT's big plain GEMMs go to the persistent kernel; invalid arguments are refused with a message, not launched
    import ctypes
    ops_mod, hip_lib = sub("ops"), sub("hip_lib")
    L = hip_lib.lib()
    meta = lambda *s_, dt=torch.bfloat16: torch.empty(*s_, dtype=dt, device="meta")
    fill = lambda **kw: ops_mod.fill_gemm_args(meta(291600, 2560), meta(7680, 2560), meta(291600, 7680), N=7680, K=2560,
                                               ptr=lambda t: 0x100000, **kw)[0]
    assert hip_lib.KERNEL_CLASSES[L.svr_gemm_kernel_class(ctypes.byref(fill()))] == "gemm_persistent"
    a = fill()
    a.epilogue = 9
    assert L.svr_gemm_kernel_class(ctypes.byref(a)) == -1 and b"unknown epilogue" in L.svr_last_error()
    a = fill(resid=meta(291600, 7680, dt=torch.float32))                  # a residual without the residual epilogue
    assert L.svr_gemm_kernel_class(ctypes.byref(a)) == -1 and b"RESID_GATE" in L.svr_last_error()


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_zero_operand_cases_route_to_the_kernel_classes_they_name():
    """tests/conditioning_cases.py ZERO_OPERAND_CASES (the epilogue sweeps of tests/test_gpu_conditioning.py) name a kernel class per
    geometry, the (output, residual) storage kinds it has a form for and who serves its activation epilogues: asked of the library's
    own routing function on shape-only tensors, so that the GPU tests cannot drift onto another kernel unnoticed.  The LDS-halo
    kernel's epilogue has no tanh-GELU: such a launch must NOT be routed to it (it would store bias-only values)."""
    import ctypes
    import conditioning_cases as cc
    from ops_reference import EPI_RESID_GATE, EPI_SWIGLU
    ops_mod, hip_lib = sub("ops"), sub("hip_lib")
    L = hip_lib.lib()

    def route(spec, out_kind, **epi):
        for k, v in {**cc.OPTION_DEFAULTS, **spec.get("options", {})}.items():
            assert L.svr_set_option(k.encode(), v) == 0
        try:
            A, W, kw, shape = cc.zero_operand_problem(spec, ops_mod, "meta", frag=lambda kind, W, s: torch.empty(W.numel(), dtype=torch.bfloat16, device="meta"))
            out = torch.empty(shape, dtype=cc.STORE_KINDS[out_kind], device="meta")
            if "resid" in epi:
                epi["resid"] = torch.empty(shape, dtype=cc.STORE_KINDS[epi["resid"]], device="meta")
            a, _ = ops_mod.fill_gemm_args(A, W, out, bias=torch.empty(kw["N"], dtype=torch.float32, device="meta"), out_f32=out_kind != "bf16",
                                          ptr=lambda t: 0x100000, zeros_ptr=0x100000, **kw, **epi)
            return hip_lib.KERNEL_CLASSES.get(L.svr_gemm_kernel_class(ctypes.byref(a)), "error")
        finally:
            for k, v in cc.OPTION_DEFAULTS.items():
                L.svr_set_option(k.encode(), v)

    for name, spec in cc.ZERO_OPERAND_CASES.items():
        for kind in cc.STORE_KINDS:
            assert route(spec, kind) == spec["cls"], (name, kind)
        pairs = spec.get("pairs")
        for o in cc.STORE_KINDS:
            for r in cc.STORE_KINDS:
                served = route(spec, o, epilogue=EPI_RESID_GATE, resid=r)
                assert (served == spec["cls"]) == (pairs is None or (o, r) in pairs), (name, o, r, served)
        for epi, cls in spec["acts"].items():
            for kind in spec.get("act_kinds", cc.STORE_KINDS):
                assert route(spec, kind, epilogue=epi) == cls, (name, epi, kind)
        if "mnk" in spec:
            assert route(spec, "bf16", epilogue=EPI_SWIGLU) == spec["cls"], name


def test_product_package_never_touches_the_oracle():
    """oracle/ (incl. the byte-compiled reference under oracle/_ref) is test infrastructure: nothing in the product package or
    the CLI may import, open or execute it -- only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do."""
    pkg = os.path.join(ROOT, "comfyui-seedvr2_videoupscaler_amd")
    files = [os.path.join(pkg, f) for f in os.listdir(pkg) if f.endswith(".py")] + [os.path.join(ROOT, "inference_cli.py")]
    files += [os.path.join(pkg, "csrc", f) for f in os.listdir(os.path.join(pkg, "csrc")) if f.endswith((".hip", ".h"))]
    for path in files:
        src = open(path).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), path
        assert "oracle/_ref" not in src and "_ref" + os.sep not in src and "reference_loader" not in src, path
    bench = open(os.path.join(ROOT, "bench.py")).read()
    uses = [m.start() for m in re.finditer(r"from oracle import|import oracle", bench)]
    assert 1 <= len(uses) <= 2
    for u in uses:                                          # each inside a top-level function named cpu_baseline* (the CPU legs)
        enclosing = bench.rfind("\ndef ", 0, u)
        assert bench.startswith("\ndef cpu_baseline", enclosing), bench[enclosing:enclosing + 60]


def test_entry_points_refuse_invalid_arguments_before_any_launch():
    """Argument validation of the elementwise entry points runs on the host before the launch, so it is checked here without a
    GPU: every call below must return non-zero and leave a message naming the entry point (never reach hipLaunchKernelGGL,
    never divide by a zero group count on the host)."""
    import ctypes
    hip_lib = sub("hip_lib")
    L = hip_lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    pf = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))
    pd = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    pi = ctypes.cast(buf, ctypes.POINTER(ctypes.c_int32))
    ph = ctypes.cast(buf, ctypes.POINTER(ctypes.c_int16))
    cases = [
        ("svr_rmsnorm_mod", lambda: L.svr_rmsnorm_mod(p, p, 4, 2560, 1e-6, None, None, None, 2, None)),      # h16 is not a stream format
        ("svr_rmsnorm_mod", lambda: L.svr_rmsnorm_mod(None, p, 4, 2560, 1e-6, None, None, None, 0, None)),
        ("svr_rmsnorm_mod", lambda: L.svr_rmsnorm_mod(p, p, 4, 2564, 1e-6, None, None, None, 0, None)),
        ("svr_ada_combine", lambda: L.svr_ada_combine(p, p, pi, pf, 70000, 2560, None)),
        ("svr_qknorm_rope", lambda: L.svr_qknorm_rope(p, 8, 20, ph, 0, pf, pf, 16, 0, pf, pf, 1e-6, None)),
        ("svr_qknorm_rope", lambda: L.svr_qknorm_rope(p, 8, 20, None, 0, pf, pf, 16, 21, pf, pf, 1e-6, None)),
        ("svr_rows_mean", lambda: L.svr_rows_mean(p, p, 3, 70000, 2560, None)),
        ("svr_patchify", lambda: L.svr_patchify(p, p, 2, 4, 6, 33, 128, None)),
        ("svr_unpatchify_euler", lambda: L.svr_unpatchify_euler(p, 32, None, p, 2, 4, 6, 16, None)),
        ("svr_groupnorm_stats", lambda: L.svr_groupnorm_stats(p, pd, p, 2, 64, 128, 0, 0, None)),            # zero groups: no host SIGFPE
        ("svr_groupnorm_stats", lambda: L.svr_groupnorm_stats(p, pd, p, 2, 64, 0, 32, 0, None)),
        ("svr_groupnorm_apply", lambda: L.svr_groupnorm_apply(p, p, pd, pf, pf, 2, 64, 128, 0, 1e-6, 1, 0, None)),
        ("svr_groupnorm_apply", lambda: L.svr_groupnorm_apply(p, p, pd, pf, pf, 2, 64, 128, 32, 1e-6, 1, 3, None)),
        ("svr_groupnorm_reduce", lambda: L.svr_groupnorm_reduce(None, pd, 2, 4, 32, None)),
        ("svr_softmax_rows", lambda: L.svr_softmax_rows(pf, p, 4, 66000, 66000, 66000, 1.0, None)),
        ("svr_blend_accumulate", lambda: L.svr_blend_accumulate(p, pf, pf, pf, pf, 1, 8, 8, 4, 8, 8, 1, 0, None)),
        ("svr_blend_finalize", lambda: L.svr_blend_finalize(pf, pf, p, 1, 64, 4, 8, 1.0, 0.0, None)),
        ("svr_affine_slice", lambda: L.svr_affine_slice(p, p, 4, 16, 32, 1.0, 0.0, None)),
        ("svr_gemm_pack_frag", lambda: L.svr_gemm_pack_frag(p, p, 100, 64, None)),
        ("svr_conv_pack_frag_taps", lambda: L.svr_conv_pack_frag_taps(p, p, 128, 100, 1, 2, 2, 32, None)),
        ("svr_set_option", lambda: L.svr_set_option(b"no_such_knob", 1)),
    ]
    for name, call in cases:
        assert call() != 0, name
        assert name.encode() in L.svr_last_error(), (name, L.svr_last_error())
