import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "comfyui-seedvr2_videoupscaler_amd"
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: multi-minute CPU test")
    config.addinivalue_line("markers", "variants: GPU tests of non-default kernel variants (opt-in: -m variants; also carry the gpu marker)")


def pytest_collection_modifyitems(config, items):
    """`-m gpu` (the driver's round-end run) spends its seconds on the shipped path: tests marked `variants` (non-default kernel
    generations / pure A-B knobs) run only when the -m expression names them (`-m variants`).  Every kernel production can still
    REACH stays in the default set: the first-generation attention kernel through test_attn_varlen's 2049-row window and its
    head_dim-512 case (and the config-2 VAE attention test with attn_as_gemm off), the generic implicit-GEMM conv through the
    strided / 1x1x1 / ragged-Cout rows of CONV_CASES under conv_impl 0, the run-time conv epilogue body through the fp32-trunk
    option sets of tests/test_gpu_wide_trunk.py.  What `variants` holds is only what no default route selects: conv_impl 1 on
    3x3 stride-1 shapes, conv_rows 4, the LDS-weight halo kernel, attn_impl 1 on windows the second kernel serves."""
    if "variants" not in (config.getoption("-m") or ""):
        keep, drop = [], []
        for it in items:
            (drop if it.get_closest_marker("variants") else keep).append(it)
        if drop:
            config.hook.pytest_deselected(items=drop)
            items[:] = keep
    _start_measurement_build(config, items)


MEASUREMENT_TEST = "test_measurement_build_compiles"


def _start_measurement_build(config, items):
    """The -DSVR_ABLATIONS device pass (tests/test_kernel_resources.py::test_measurement_build_compiles) takes three minutes of one
    core: when that test is part of the run, its compile is started NOW, in the background, the test is moved to the end of the
    run and only collects the result -- the suite's other minutes hide it."""
    if getattr(config, "workerinput", None) is not None:      # (pytest-xdist worker: let the test compile inline)
        return
    mine = [it for it in items if it.name == MEASUREMENT_TEST]
    marker = config.getoption("-m") or ""
    if not mine or ("not gpu" not in marker and marker) or config.getoption("collectonly", False):
        return                                                 # (a GPU-only selection deselects the test later; --collect-only runs nothing)
    import shutil
    import subprocess
    import tempfile
    hip_lib = importlib.import_module(f"{PKG}.hip_lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        return
    out = os.path.join(tempfile.mkdtemp(prefix="svr_abl_"), "svr_api_ablations.s")
    cmd = [hipcc] + [f for f in hip_lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + \
          ["-DSVR_ABLATIONS", "-S", "--cuda-device-only", os.path.join(hip_lib.CSRC, "svr_api.hip"), "-o", out]
    # (own process group: hipcc runs clang++ through a shell, and an interrupted run must be able to take all of them down)
    config._svr_measurement_build = (subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                                                      start_new_session=True), out)
    items[:] = [it for it in items if it.name != MEASUREMENT_TEST] + mine
    # the compile keeps one core busy for ~5 minutes: with as many OpenMP threads as cores every parallel region of the tests running
    # next to it waits for the thread that shares that core (measured: 5-15x per test, 12 instead of 7 minutes for the suite), so the
    # tests leave it one core
    try:
        import torch
        torch.set_num_threads(max(1, torch.get_num_threads() - 1))
    except Exception:                                            # noqa: BLE001 (a thread-count hint must never fail a run)
        pass


def pytest_unconfigure(config):
    _save_recorded()
    job = getattr(config, "_svr_measurement_build", None)
    if job is not None and job[0].poll() is None:              # (run interrupted before the test collected it: do not leave it behind)
        import signal
        try:
            os.killpg(job[0].pid, signal.SIGTERM)
        except OSError:
            job[0].kill()


def sub(name):
    return importlib.import_module(f"{PKG}.{name}" if name else PKG)


@pytest.fixture(scope="session")
def pkg():
    return importlib.import_module(PKG)


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------ recorded reference results
# A test that compares against the reference's own code runs that code where it is available (oracle/reference_loader.py: the
# checkout or oracle/_ref) and, everywhere else, compares against the results such a run recorded: tests/golden/recorded_<group>.pt,
# written by `SVR_RECORD_REFERENCE=1 pytest ...` where the reference is available.  A result that was never recorded fails.
RECORD = os.environ.get("SVR_RECORD_REFERENCE") == "1"
_recorded, _recorded_dirty = {}, set()


def _recorded_path(group):
    return os.path.join(GOLDEN, f"recorded_{group}.pt")


def _owned(value):
    """Tensors cloned (a view would save its whole storage), containers rebuilt."""
    import torch
    if isinstance(value, torch.Tensor):
        return value.detach().clone()
    if isinstance(value, (list, tuple)):
        return type(value)(_owned(v) for v in value)
    if isinstance(value, dict):
        return {k: _owned(v) for k, v in value.items()}
    return value


def recorded(group, key, live):
    """The reference's result ``live()`` where the reference is available (stored when recording), else the recorded one."""
    import torch
    from oracle import reference_loader as rl
    if group not in _recorded:
        path = _recorded_path(group)
        _recorded[group] = torch.load(path, weights_only=True) if os.path.exists(path) else {}
    table = _recorded[group]
    if rl.available():
        value = live()
        if RECORD:
            table[key] = _owned(value)
            _recorded_dirty.add(group)
        return value
    assert key in table, f"{key!r} is not recorded in {_recorded_path(group)}: record it where the reference is available (SVR_RECORD_REFERENCE=1)"
    return table[key]


def _save_recorded():
    import torch
    for group in sorted(_recorded_dirty):
        torch.save(_recorded[group], _recorded_path(group))
    _recorded_dirty.clear()


def digest(t):
    """Bit pattern, shape and dtype of a tensor as one string: bit-exact comparison with a recorded result too large to store."""
    import hashlib
    import torch
    t = t.detach().contiguous().cpu()
    return f"{tuple(t.shape)} {t.dtype} " + hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
