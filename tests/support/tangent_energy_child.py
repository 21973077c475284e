"""Child process of tests/test_tangent_energy_gpu.py:

    python tangent_energy_child.py partitioned    the refusals of a handle with an exchange (fc_set_host_exchange)

Prints CHILD OK <mode> at the end; exits non-zero with the failed assertion."""
import sys

import numpy as np


def main(mode: str) -> None:
    if mode == "partitioned":
        from flowcontrol_amd import _lib
        from flowcontrol_amd.device import DeviceSolver
        from flowcontrol_amd.fem.mesh import Mesh
        from flowcontrol_amd.fem.spaces import TaylorHood

        dev = DeviceSolver(TaylorHood(Mesh.unit_square(4, 4)))
        try:
            fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
            _lib.check(dev.lib.fc_set_host_exchange(dev._h, 2, 0, fn, None))
            calls = {"fc_tangent_set_energy": lambda: dev.lib.fc_tangent_set_energy(dev._h, 1),
                     "fc_tangent_tape_reserve": lambda: dev.lib.fc_tangent_tape_reserve(dev._h, 4),
                     "fc_set_adjoint_energy_source": lambda: dev.lib.fc_set_adjoint_energy_source(dev._h, 1)}
            for name, call in calls.items():
                code, msg = call(), dev.lib.fc_last_error().decode()
                assert code == _lib.FC_ERR_INVALID and name in msg and "partitioned" in msg, (name, code, msg)
            assert dev.lib.fc_get_tangent_energy(dev._h, 1, 0, np.zeros(1)) == _lib.FC_ERR_NOT_READY
            info = dev.tangent_energy_info()
            assert not info["on"] and info["bytes"] == 0 and dev.tangent_info()["bytes"] == 0
            assert dev.tangent_tape_info()["bytes"] == 0
        finally:
            dev.close()
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    print("CHILD OK", mode, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
