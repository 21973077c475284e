"""The backward schedule of the adjoint marches (``csrc/fc_adjoint_schedule.hpp``) without a GPU: a stand-alone C++ program, built with
the address and undefined-behaviour sanitizers, compares slot, coefficients, tape column and energy row of every backward step and of
the two state-gradient products with a table collected from the forward recurrence, exactly, for n_steps = 1, 2, 3, 4, 7, both first
slots and linearised and nonlinear coefficient sets."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flowcontrol_amd" / "csrc" / "fc_adjoint_schedule.hpp"


def test_schedule_against_the_forward_recurrence(tmp_path):
    exe = tmp_path / "adjoint_schedule_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), str(ROOT / "tests" / "support" / "adjoint_schedule_host_check.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "CHECK OK"
    assert not [ln for ln in lines if "FAILED" in ln]
    checks = {ln[:-len(" ok")] for ln in lines if ln.endswith(" ok")}
    want = {f"{kind}_bdf{first}_n{n}_{part}" for kind in ("lin", "nl", "distinct") for first in (1, 2) for n in (1, 2, 3, 4, 7)
            for part in ("steps", "dx0", "dxm1")}
    assert checks == want


def test_the_header_is_host_only():
    """Nothing in it includes HIP (it is compiled by g++ above) or another project header, and nothing names the device."""
    text = HEADER.read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert all(inc.startswith("<") and "hip" not in inc for inc in includes), includes
    assert "__device__" not in text and "__global__" not in text and "hipStream" not in text
