"""The launch dispatcher (``csrc/fc_dispatch.hpp``) without a GPU: a small C++ driver sends every entry of every instance list, and
their neighbours, through the pickers; the lists it prints are the ones ``tests/support`` restates by hand."""
import subprocess
from pathlib import Path

from tests.support import batch_cases as bc
from tests.support import sweep_cases as sc

ROOT = Path(__file__).resolve().parents[1]

#: list of the header -> the constant the route tests enumerate their cases from
RESTATED = {
    "BatchWidths": bc.KBS,
    "SweepGeoms": sc.SWEEP_KEYS,
    "BlockDownGeoms": sc.BLOCK_DOWN_KEYS,
    "BlockUpColumnGeoms": sc.BLOCK_UPC_KEYS,
    "FlatLoads": sc.FLAT_LOADS,
    "SweepGeomsCompressed": tuple(sc.LP_SWEEP.items()),
    "BlockGeomsCompressed": tuple(sc.LP_BLOCK.items()),
}
#: lane lists of the CSR products (nothing restates them); the last entry is the instance any other lane count falls through to
LANES = {"SpmvLanes": (4, 8, 16, 32, 64), "PcLanes": (1, 4, 8, 16, 32), "ShiftedSpmvLanes": (8, 16, 32)}


def test_pickers_and_instance_lists(tmp_path):
    exe = tmp_path / "dispatch_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "tests" / "support" / "dispatch_host_check.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lists, tried = {}, {}
    for line in out.strip().splitlines():
        f = line.split()
        if f[0] == "list":
            assert f[1] not in lists, line
            lists[f[1]] = [tuple(int(x) for x in e.split(":")) if ":" in e else int(e) for e in f[2:]]
        else:
            name, what, passed, n = f[0], f[1], int(f[2]), int(f[3])
            assert passed == n and n > 0, line
            tried[(name, what)] = n
    assert set(lists) == set(RESTATED) | set(LANES)
    for name, want in {**RESTATED, **LANES}.items():
        assert len(lists[name]) == len(want) and set(lists[name]) == set(want), name
        # every entry reached the functor once; pair lists were also tried transposed
        assert tried[(name, "hit")] == len(want) and tried[(name, "miss")] > 0, name
        if isinstance(lists[name][0], tuple):
            assert tried[(name, "transposed")] == sum((b, a) not in want for a, b in want), name
    for name in LANES:
        assert lists[name][-1] == max(lists[name]), name
    assert tried[("Bool", "hit")] == 2 and tried[("Empty", "miss")] == 1
    # the example of a transposed pair: (8, 4) is a sweep geometry, (4, 8) is not
    assert (8, 4) in lists["SweepGeoms"] and (4, 8) not in lists["SweepGeoms"]
    # the down form has no instance for the small nodes' geometries of the column form
    assert set(lists["BlockUpColumnGeoms"]) - set(lists["BlockDownGeoms"]) == {(8, 1), (8, 2), (16, 4)}
