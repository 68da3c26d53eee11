"""Run a golden comparison with the float32 elementary functions the goldens were recorded with.

torch evaluates float32 exp / log on the CPU with MKL's vector math, and MKL's default code path depends on the CPU: on an
AVX-512 Intel host and on an AMD host exp / log differ in the last bit.  The schedule and sinusoid goldens (tests/golden/g1*,
g2) are therefore recorded on MKL's CPU-independent path (conditional numerical reproducibility, MKL_CBWR=COMPATIBLE:
tests/golden/make_goldens.py), and a test decorated with @recorded_math runs in a child pytest process pinned to that
same path.  Its assertions are unchanged and stay bit for bit; the pin stays in the child, other tests keep MKL's default."""
import functools
import inspect
import os
import subprocess
import sys
from pathlib import Path

MKL_ENV = {"MKL_CBWR": "COMPATIBLE"}
_CHILD = "RECORDED_MATH_CHILD"


def recorded_math(test):
    @functools.wraps(test)
    def run(*args, **kwargs):
        if os.environ.get(_CHILD):
            return test(*args, **kwargs)
        node = f"{inspect.getfile(test)}::{test.__name__}"
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", node], capture_output=True, text=True,
                           timeout=900, cwd=Path(__file__).resolve().parent.parent, env=dict(os.environ, **MKL_ENV, **{_CHILD: "1"}))
        assert r.returncode == 0, f"{node} with {MKL_ENV}:\n{r.stdout[-6000:]}{r.stderr[-2000:]}"
    return run
