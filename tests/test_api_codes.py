"""The C ABI's return codes on CPU: tools/asan_host_check.py drives every
validation path of liblsr.so (each call rejected, or a no-op, before any HIP
call) and asserts the code each returns, including which of two failing checks
wins.  Here it runs against the regular build in a fresh child process (the
sanitizer job, tests/test_asan.py, runs the same table on the instrumented
build)."""
import os
import re
import subprocess
import sys

from langsplatv2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_return_code_table():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "langsplatv2_amd", "csrc")], check=True,
                       timeout=1800)
    env = dict(os.environ, LSR_LIB=_lib.LIB_PATH)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asan_host_check.py")], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert re.search(r"^ok \d+$", p.stdout, flags=re.M), p.stdout[-1000:]
