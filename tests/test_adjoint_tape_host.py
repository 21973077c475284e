"""The host bookkeeping of the dense adjoint state tape -- the one-segment form of ``csrc/fc_adjoint_segments.hpp`` -- without a GPU: a
stand-alone C++ program, built with the address and undefined-behaviour sanitizers, drives begin / push / pop / invalidate / overflow
sequences and the "covers this run" query with every refusal reason, then compares the one-segment form with a model of the dense tape
over seeded random sequences, field by field after every operation."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

#: the reasons covers() can give, each with a word its text must carry
REFUSALS = {"none": "no tape", "not_begun": "not begun", "overflowed": "overflowed", "count": "holds 3 steps", "first_slot": "first taped step",
            "later_slot": "taped step 3"}


def test_tape_bookkeeping(tmp_path):
    exe = tmp_path / "adjoint_tape_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "flowcontrol_amd" / "csrc"), str(ROOT / "tests" / "support" / "adjoint_tape_host_check.cpp"), "-o", str(exe)],
                   check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "CHECK OK"
    checks = [ln for ln in lines if ln.endswith(" ok")]
    assert len(checks) >= 30 and not [ln for ln in lines if "FAILED" in ln]
    assert "model_comparison ok" in checks and "model comparison: 1200000 operations" in lines
    reasons = dict(ln[len("refusal "):].split(": ", 1) for ln in lines if ln.startswith("refusal "))
    assert set(reasons) == set(REFUSALS)
    for key, word in REFUSALS.items():
        assert word in reasons[key], (key, reasons[key])


def test_the_header_is_host_only():
    """Nothing in it includes HIP (it is compiled by g++ above) or another project header."""
    text = (ROOT / "flowcontrol_amd" / "csrc" / "fc_adjoint_segments.hpp").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes
