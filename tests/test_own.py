"""The context's resource owners (csrc/hpe_own.hpp) on the CPU: tools/own_check.cpp instantiates
DevBuf, HostBuf, Event and Stream on a fake allocator that counts what is live and fails its n-th
call, and runs the all-or-nothing shapes the ensure_* functions build from them -- moves,
self-moves, reset, alloc(0), a vector of slots growing, and every group allocation with the
failure injected at every call in turn.  No GPU, no HIP runtime."""
import subprocess

import hand_data


def test_own_check_tool():
    pkg = hand_data.ROOT / "hand-pose-estimation_amd"
    subprocess.run(["make", "-C", str(pkg), "own_check"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([str(pkg / "own_check")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "own_check: ok" in r.stdout and "FAIL" not in r.stdout
