"""The checkpointed state tape's host bookkeeping (``csrc/fc_adjoint_segments.hpp``) without a GPU: a stand-alone C++ program, built
with the address and undefined-behaviour sanitizers, walks every run length n = 1 .. 40 with every spacing c = 1 .. n + 2 over a store of
state INDICES and prints where each forward step wrote, which buffer column each backward step read and which segments were replayed;
this file restates those tables on its own, from the layout alone (checkpoint j = (x_{jc-1}, x_{jc}); buffer column i + 1 = x_{jc+i})."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "flowcontrol_amd" / "csrc" / "fc_adjoint_segments.hpp"


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("segments") / "adjoint_segments_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), str(ROOT / "tests" / "support" / "adjoint_segments_host_check.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout.strip().splitlines()


def restated(n, c):
    """(columns, replayed, forward writes, march reads, segments) of a run of n steps with spacing c."""
    segs = -(-n // c)
    writes = []
    for m in range(1, n + 1):
        j, i = divmod(m - 1, c)  # step m is step i + 1 of segment j: x_{jc+i+1} -> column i + 2
        writes.append((i + 2, j if (i == 0 and j > 0) else -1))
    last_len = n - (segs - 1) * c
    march = [(m, m + 1 - ((m - 1) // c) * c) for m in range(n, 0, -1)]
    replay = [(j, 0 if j == segs - 1 else 1) for j in range(segs - 1, -1, -1)]
    return 2 * segs + c + 2, n - last_len, writes, march, replay


def test_every_run_length_and_spacing(output):
    assert output[-1] == "CHECK OK"
    assert not [ln for ln in output if "FAILED" in ln]
    cases = {}
    for ln in output:
        if not ln.startswith("case "):
            continue
        head, writes, march, segs = (part.split() for part in ln.split("|"))
        pairs = lambda items: [tuple(int(v) for v in it.split(":")) for it in items]  # noqa: E731
        cases[(int(head[1]), int(head[2]))] = (int(head[3]), int(head[4]), pairs(writes), pairs(march), pairs(segs))
    want = {(n, c) for n in range(1, 41) for c in range(1, n + 3)}
    assert set(cases) == want
    for n, c in sorted(want):
        assert cases[(n, c)] == restated(n, c), (n, c)
    ok = {ln[:-len(" ok")] for ln in output if ln.endswith(" ok")}
    assert {f"case_n{n}_c{c}" for n, c in want} <= ok


def test_memory_formula():
    """Columns held against the dense tape's n + 2, and the spacing that minimises them."""
    import math

    for n in (7, 1000, 10000):
        best = min(range(1, n + 1), key=lambda c: 2 * -(-n // c) + c)
        auto = math.isqrt(2 * n - 1) + 1  # ceil(sqrt(2 n))
        assert auto == math.ceil(math.sqrt(2 * n))
        assert 2 * -(-n // auto) + auto <= 2 * -(-n // best) + best + 2
    assert restated(1000, 45)[0] == 2 * 23 + 47 and restated(1000, 45)[0] * 10 < 1002


def test_push_pop_overflow_and_covers_messages(output):
    ok = {ln[:-len(" ok")] for ln in output if ln.endswith(" ok")}
    for name in ("none_push", "none_begin", "none_covers", "every_zero", "capacity_zero", "reserved_columns", "reserved_push", "reserved_covers",
                 "begin", "push_columns", "overflow", "overflow_covers", "pop_lost", "count_covers", "first_slot_covers", "pop_across_boundary",
                 "pop_inside", "pop_inside_column", "later_slot_covers", "pop_to_begin", "pop_before_begin", "marched_next", "marched_push",
                 "marched_pop", "one_segment", "one_segment_goes_on", "invalidate", "begin_again", "release", "negative_capacity"):
        assert name in ok, name
    why = {ln.split(":", 1)[0][len("refusal "):]: ln.split(":", 1)[1].strip() for ln in output if ln.startswith("refusal ")}
    # the dense tape's wording (tests/support/adjoint_tape_host_check.cpp holds its model)
    assert why["none"] == "no tape is reserved"
    assert why["not_begun"].startswith("the tape is not begun")
    assert why["overflowed"] == "the tape overflowed: 4 steps since it was begun, capacity 3"
    assert why["count"] == "the tape holds 3 steps, the run has 2"
    assert why["first_slot"] == "the first taped step ran on order slot 0, not on 1"
    assert why["later_slot"] == "taped step 2 ran on order slot 0, not on 1"


def test_the_header_is_host_only():
    text = HEADER.read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert all(inc.startswith("<") and "hip" not in inc for inc in includes), includes
    assert "__device__" not in text and "__global__" not in text and "hipStream" not in text
