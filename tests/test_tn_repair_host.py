"""In-stream repair of tripped weight-gradient products (include/tfgnn.h tfgnn_sp_guard_repair), the part that needs no GPU:
the two new symbols are exported, declared and bound, the ABI number did not move, the switch is off unless the environment
arms it, and the workspace queries grow by exactly the 256-byte tail of the trip word while it is armed."""
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_sp_guard_repair", "tfgnn_sp_repair_stats"]
SHAPES = [(256, 128, 2017, 256, 64), (640, 128, 6053, 640, 320), (1280, 320, 30000, 1280, 320)]


def test_new_symbols_are_exported_declared_and_bound_and_the_abi_stays_5():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    table = {row[0] for row in _lib._SIGNATURES}
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in table and name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5
    assert "#define TFGNN_ABI_VERSION 5" in text


def _sizes_in_child(env_value):
    code = (
        "from tf2_gnn_amd import _lib\n"
        "lib = _lib.load()\n"
        "print('STATE', lib.tfgnn_sp_guard_repair(-1))\n"
        f"for s in {SHAPES!r}:\n"
        "    print('BYTES', lib.tfgnn_sp_gemm_tn_workspace_bytes(*s), lib.tfgnn_sp_gemm_tn_wide_workspace_bytes(*s))\n"
    )
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("TFGNN_GUARD_REPAIR", None)
    if env_value is not None:
        env["TFGNN_GUARD_REPAIR"] = env_value
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    lines = res.stdout.splitlines()
    state = [int(l.split()[1]) for l in lines if l.startswith("STATE")]
    sizes = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("BYTES")]
    assert len(state) == 1 and len(sizes) == len(SHAPES)
    return state[0], sizes


def test_the_switch_follows_the_environment_and_adds_exactly_the_trip_word_tail():
    """The state is read from TFGNN_GUARD_REPAIR once per process (hence child processes); querying it and the sizes touches no
    device."""
    off_state, off = _sizes_in_child(None)
    zero_state, zero = _sizes_in_child("0")
    on_state, on = _sizes_in_child("1")
    assert (off_state, zero_state, on_state) == (0, 0, 1)
    assert off == zero
    for (p0, w0), (p1, w1) in zip(off, on):
        assert p0 > 0 and w0 >= p0 and p0 % 256 == 0 and w0 % 256 == 0
        assert (p1, w1) == (p0 + 256, w0 + 256)
