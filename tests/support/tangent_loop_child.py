"""Child process of tests/test_tangent_loop_gpu.py -- TEST INFRASTRUCTURE:

    python tangent_loop_child.py partitioned    both closed-loop tangent marches refuse a handle with an exchange (fc_set_host_exchange)

Prints CHILD OK <mode> at the end; exits non-zero with the failed assertion."""
import sys


def main(mode: str) -> None:
    if mode != "partitioned":
        raise SystemExit(f"unknown mode {mode!r}")
    from flowcontrol_amd import _lib
    from flowcontrol_amd._lib import SLOT_BDF2
    from flowcontrol_amd.device import DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    dev = DeviceSolver(TaylorHood(Mesh.unit_square(4, 4)))
    try:
        fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
        _lib.check(dev.lib.fc_set_host_exchange(dev._h, 2, 0, fn, None))
        nul = [None] * 18
        calls = {"fc_run_tangent_closed_loop": lambda: dev.lib.fc_run_tangent_closed_loop(dev._h, SLOT_BDF2, 2, *nul),
                 "fc_run_tangent_closed_loop_batch": lambda: dev.lib.fc_run_tangent_closed_loop_batch(dev._h, SLOT_BDF2, 4, 2, -1, *nul, None)}
        marches = dev.tangent_info()["marches"]
        for name, call in calls.items():
            code, msg = call(), dev.lib.fc_last_error().decode()
            assert code == _lib.FC_ERR_INVALID and name in msg and "partitioned" in msg, (name, code, msg)
        assert dev.tangent_info()["marches"] == marches and dev.tangent_info()["bytes"] == 0
    finally:
        dev.close()
    print("CHILD OK", mode, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
