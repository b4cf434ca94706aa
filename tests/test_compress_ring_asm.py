"""Build-time check of k_compress_fast's hand-issued input-ring loads (no GPU needed)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compress_ring_loads_are_not_touched_before_their_wait():
    """tools/check_compress_ring_asm.py: the ring register in flight across windows must not be read, copied or spilled
    by compiler code before a `vmcnt(0)` drains it, in every instantiation of k_compress_fast (re-run after any toolchain
    change)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_compress_ring_asm.py")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 problems" in out.stdout and "7 kernels" in out.stdout, out.stdout
