"""The step-record protocol (``csrc/fc_record.hpp``: layout, checksum fold, the host's readers) without a GPU: a small C++ driver
builds step records and late records with the fold the kernels use and hands them, intact and damaged, to the readers that
``fc_hip.hip`` calls."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

#: damaged records: none may be accepted
REJECTED = {"step_stale_seq", "step_payload_word", "step_checksum_word", "step_exchanged",
            "late_stale_seq", "late_payload_word", "late_checksum_word", "late_exchanged"}
#: intact records, also after every word the layout does not name was overwritten: all accepted
ACCEPTED = {"fold", "step_intact", "step_other_words", "late_intact", "late_other_words"}


def test_record_readers_accept_intact_and_reject_damaged(tmp_path):
    exe = tmp_path / "record_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "tests" / "support" / "record_host_check.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    tried = {}
    for line in out.strip().splitlines():
        key, accepted, n = line.split()
        accepted, n = int(accepted), int(n)
        tried[key] = tried.get(key, 0) + n
        if key in REJECTED:
            assert accepted == 0, line
        elif key in ACCEPTED:
            assert accepted == n, line
        else:
            # exchanged payload words leave the XOR as it was: the case the odd-weighted sum exists for
            assert key == "step_exchanged_xor_blind" and accepted == n, line
    assert set(tried) == REJECTED | ACCEPTED | {"step_exchanged_xor_blind"}
    # step records with 0, 1, 3 and 64 sensors (+ E, r^2, b^2, flag), four ways of damaging a word
    words = [n + 4 for n in (0, 1, 3, 64)]
    assert tried["step_intact"] == 4 and tried["late_intact"] == 1
    assert tried["step_payload_word"] == 4 * sum(words) and tried["late_payload_word"] == 4 * 4
    assert tried["step_checksum_word"] == 4 * 2 * 4 and tried["late_checksum_word"] == 2 * 4
    assert tried["step_exchanged"] == sum(w * (w - 1) // 2 for w in words) and tried["late_exchanged"] == 6
    assert tried["step_other_words"] == sum(160 - w - 3 for w in words) and tried["late_other_words"] == 1
