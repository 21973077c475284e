"""Factorisation-free Krylov mode (``fc_setup_krylov``, ``krylov_precond="schur_amg"``) on partitioned handles: every rank computes
its own rows and the root's, the SIMPLE / AMG preconditioner takes ONE exchange per apply (the root's partial velocity rows + every
rank's share of the Schur right-hand side), the pressure hierarchy is built from the matrix gathered once at setup and replicated.

Ranks share GPU 0: thread ranks (``ThreadComm``) and gloo process ranks exchange through the host; ``FC_FORCE_COMM=1`` drives the
in-stream RCCL all-reduce with a one-rank communicator."""
import os
import socket
import tempfile
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch.distributed as dist
import torch.multiprocessing as mp

from flowcontrol_amd.examples.data import mesh_file
from flowcontrol_amd.fem.mesh import read_xdmf_mesh
from flowcontrol_amd.fem.spaces import TaylorHood

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DT, RE = 0.005, 100.0


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bc(th):
    m = th.mesh
    be = m.boundary_edges()
    be = be[m.edge_midpoints()[be, 0] < m.coords[:, 0].max() - 1e-9]
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    return np.sort(np.r_[nodes, nodes + th.nn])


def _handle(comm=None):
    """O1 BDF2 operator in slot SLOT_BDF2 of a fresh handle (one rank of ``comm``, or a single GPU)."""
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver

    th = TaylorHood(read_xdmf_mesh(mesh_file("O1")))
    dev = DeviceSolver(th)
    if comm is not None:
        dev.join(comm.rank, comm.world, comm.bcast, comm.allreduce)
    x = th.node_coords
    U0 = np.r_[1.0 + 0.3 * np.sin(x[:, 0]) * np.cos(0.7 * x[:, 1]), 0.2 * np.cos(0.5 * x[:, 0] + 0.1) * np.sin(x[:, 1])]
    dofs = _bc(th)
    dev.set_bc(dofs, np.zeros((dofs.size, 1)))
    dev.assemble_matrix(SLOT_BDF2, mass=1.5 / DT, nu=1.0 / RE, adv=U0, lin=U0)
    dev.apply_bc(SLOT_BDF2)
    return th, dev, dofs


def _vectors(N, dofs):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(N)
    b = rng.standard_normal(N)
    b[dofs] = 0.0
    return x, b


def _rank_apply(comm, method):
    from flowcontrol_amd.device import SLOT_BDF2

    th, dev, dofs = _handle(comm)
    x, b = _vectors(th.N, dofs)
    info = dev.setup_krylov(SLOT_BDF2, sweeps=2, method=method, max_iter=300, rtol=1e-12)
    out = {"perm": dev.perm.copy(), "apply": dev.debug_apply_pc(SLOT_BDF2, x), "info": info, "part": dev.krylov_partition_info(SLOT_BDF2)}
    xs, si = dev.solve(SLOT_BDF2, b)
    out.update(x=xs, iters=int(si[0]), resid=float(si[1]), rowkind=dev.part.rowkind.copy())
    dev.close()
    return out


def _process_apply(rank, world, port, res, method):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowcontrol_amd.comm import default_comm

        res[rank] = _rank_apply(default_comm(), method)
    finally:
        dist.destroy_process_group()


def _single_with_perm(perm, method="gmres"):
    """The single-GPU handle with the partitioned handles' permutation: the reference for their apply and their bytes."""
    from flowcontrol_amd import _lib
    from flowcontrol_amd.device import SLOT_BDF2

    th, dev, dofs = _handle()
    x, b = _vectors(th.N, dofs)
    _lib.check(dev.lib.fc_set_permutation(dev._h, np.ascontiguousarray(perm, dtype=np.int32)))
    info = dev.setup_krylov(SLOT_BDF2, sweeps=2, method=method, max_iter=300, rtol=1e-12)
    out = {"apply": dev.debug_apply_pc(SLOT_BDF2, x), "info": info, "part": dev.krylov_partition_info(SLOT_BDF2)}
    A = dev.matrix(SLOT_BDF2).tocsc()
    out["x_direct"] = spla.splu(A).solve(b)
    out["A"] = A.tocsr()
    dev.close()
    return out


@pytest.mark.parametrize("world,ranks", [(2, "process"), (4, "thread"), (8, "thread")])
def test_distributed_apply_and_solve_equal_the_single_gpu_ones(world, ranks):
    """Per rank: the merged apply equals the single handle's (same permutation) to 1e-13; the same omega, AMG levels, coarse rows and
    pressure dofs on every rank; one exchange per apply; GMRES to SuperLU's solution with the same residual and iteration count on
    every rank; the rows the ranks compute tile the single handle's, the root's counted once per rank; rank-local bytes within
    1.35 x the single handle's / world plus what the root's velocity rows carry; replicated bytes = the single handle's hierarchy."""
    from flowcontrol_amd.comm import run_threaded

    if ranks == "thread":
        outs = run_threaded(world, _rank_apply, "gmres")
    else:
        with mp.Manager() as mgr:
            res = mgr.dict()
            mp.spawn(_process_apply, args=(world, _free_port(), res, "gmres"), nprocs=world, join=True)
            outs = [dict(res[r]) for r in range(world)]
    ref = _single_with_perm(outs[0]["perm"])
    A = ref["A"]
    nn2 = A.shape[0] - ref["info"]["pressure_dofs"]
    root = np.flatnonzero(outs[0]["rowkind"] == 2)  # W numbering
    root_v, n_root_p = root[root < nn2], int(np.count_nonzero(root >= nn2))
    # what a root velocity row can add to a rank's share: its K_F row and its Bt row (both within its row of A) and B's entries in its
    # column (within its column of A), 12 bytes per entry, plus a row pointer in K_F and Bt
    At = A.T.tocsr()
    root_allowance = 12 * int(2 * np.diff(A.indptr)[root_v].sum() + np.diff(At.indptr)[root_v].sum()) + 8 * root_v.size
    for o in outs:
        assert np.array_equal(o["perm"], outs[0]["perm"]) and np.array_equal(o["rowkind"] == 2, outs[0]["rowkind"] == 2)
        assert _rel(o["apply"], ref["apply"]) <= 1e-13, _rel(o["apply"], ref["apply"])
        assert o["info"]["jacobi_omega"] == outs[0]["info"]["jacobi_omega"]  # bit-equal on every rank
        assert abs(o["info"]["jacobi_omega"] - ref["info"]["jacobi_omega"]) <= 1e-14 * ref["info"]["jacobi_omega"]
        for k in ("amg_levels", "coarsest_rows", "pressure_dofs"):
            assert o["info"][k] == ref["info"][k], k
        p = o["part"]
        assert p["exchanges_per_apply"] == 1 and p["root_rows"] == root.size
        assert p["doubles_per_apply"] == root_v.size + ref["info"]["pressure_dofs"]
        assert p["replicated_bytes"] == ref["part"]["replicated_bytes"]
        assert p["local_bytes"] <= 1.35 * ref["part"]["local_bytes"] / world + root_allowance, (p["local_bytes"], ref["part"]["local_bytes"])
        assert _rel(o["x"], ref["x_direct"]) <= 1e-10, _rel(o["x"], ref["x_direct"])
        assert o["iters"] == outs[0]["iters"] and o["resid"] == outs[0]["resid"]
    # every velocity / pressure row is computed by exactly one rank, the root's by all of them
    assert sum(o["part"]["velocity_rows"] for o in outs) == ref["part"]["velocity_rows"] + (world - 1) * root_v.size
    assert sum(o["part"]["pressure_rows"] for o in outs) == ref["part"]["pressure_rows"] + (world - 1) * n_root_p
    print(f"[world {world}, {ranks} ranks] GMRES iterations {outs[0]['iters']}, residual {outs[0]['resid']:.1e}; rank 0 holds "
          f"{outs[0]['part']['local_bytes'] / 1e6:.2f} MB local (single GPU {ref['part']['local_bytes'] / 1e6:.2f}), "
          f"{outs[0]['part']['replicated_bytes'] / 1e6:.2f} MB replicated; {outs[0]['part']['doubles_per_apply']} doubles per apply")


def test_bicgstab_on_two_thread_ranks():
    from flowcontrol_amd.comm import run_threaded

    outs = run_threaded(2, _rank_apply, "bicgstab")
    ref = _single_with_perm(outs[0]["perm"], "bicgstab")
    for o in outs:
        assert _rel(o["x"], ref["x_direct"]) <= 1e-10 and o["iters"] == outs[0]["iters"]


# ── time steps: the _worker / _serial scenario of test_partitioned_gpu.py in factor-free mode ──
def _scenario(fs, nsteps, before_steps=None):
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    if before_steps is not None:
        before_steps()
    its = []
    for k in range(nsteps):
        fs.step([0.05 * np.sin(0.3 * k), -0.02])
        its.append(int(fs.solve_info[0]))
    ts = fs.timeseries
    return {"y": ts[["y_meas_1", "y_meas_2", "y_meas_3"]].to_numpy(), "dE": ts["dE"].to_numpy(), "u": fs.fields.u_.vector().get_local(),
            "its": its, "resid": float(fs.solve_info[1])}


def _solver(nsteps, krylov):
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=nsteps)
    if krylov:
        fs.krylov_precond, fs.krylov_method, fs.krylov_max_iter, fs.krylov_rtol = "schur_amg", "gmres", 300, 1e-11
    return fs


def _serial(nsteps, krylov):
    fs = _solver(nsteps, krylov)
    out = _scenario(fs, nsteps)
    fs.th.release_device()
    return out


def _thread_rank(comm, nsteps):
    fs = _solver(nsteps, True)
    fs.comm = comm
    out = _scenario(fs, nsteps)
    dev = fs.th.device()
    out["part"] = dev.krylov_partition_info(1)
    out["cells"] = int(dev.part.local_cells.size)
    fs.th.release_device()
    return out


def _process_rank(rank, world, port, res, nsteps):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fs = _solver(nsteps, True)
        out = _scenario(fs, nsteps)
        out["part"] = fs.th.device().krylov_partition_info(1)
        res[rank] = out
        fs.th.release_device()
    finally:
        dist.destroy_process_group()


def _check_steps(outs, direct, free, nsteps):
    for o in outs:
        assert _rel(o["y"], direct["y"]) < 1e-8 and _rel(o["dE"], direct["dE"]) < 1e-8 and _rel(o["u"], direct["u"]) < 1e-8
        assert o["its"] == outs[0]["its"] and o["resid"] < 1e-9
        assert o["part"]["exchanges_per_apply"] == 1 and o["part"]["exchanges_last_step"] > 0
    assert np.mean(outs[0]["its"]) <= 1.3 * np.mean(free["its"]) + 0.5, (outs[0]["its"], free["its"])


@pytest.mark.parametrize("world,ranks", [(2, "process"), (4, "thread")])
def test_factor_free_steps_on_partitioned_ranks_follow_the_direct_run(world, ranks):
    from flowcontrol_amd.comm import run_threaded

    nsteps = 20
    direct, free = _serial(nsteps, False), _serial(nsteps, True)
    if ranks == "thread":
        outs = run_threaded(world, _thread_rank, nsteps)
    else:
        with mp.Manager() as mgr:
            res = mgr.dict()
            mp.spawn(_process_rank, args=(world, _free_port(), res, nsteps), nprocs=world, join=True)
            outs = [dict(res[r]) for r in range(world)]
    _check_steps(outs, direct, free, nsteps)
    p = outs[0]["part"]
    print(f"[world {world}, {ranks} ranks] GMRES iterations per step: mean {np.mean(outs[0]['its']):.1f} (single GPU {np.mean(free['its']):.1f}); "
          f"{p['exchanges_last_step']} exchanges in the last step's solve")


def test_rccl_plumbing_with_a_single_rank_communicator_in_factor_free_mode(monkeypatch):
    """FC_FORCE_COMM=1: the partitioned factor-free path (row kinds, the apply's in-stream all-reduce, the mat-vec's root sum, the step
    tail's record) over a one-rank RCCL communicator equals the single-GPU factor-free series."""
    nsteps = 10
    free = _serial(nsteps, True)
    monkeypatch.setenv("FC_FORCE_COMM", "1")
    fs = _solver(nsteps, True)

    def join():
        fs.th.device().join(0, 1, lambda b: b)
        fs._joined = True

    out = _scenario(fs, nsteps, join)
    dev = fs.th.device()
    assert dev.part is not None and dev.part.ar_n > 0
    assert dev.krylov_partition_info(1)["exchanges_per_apply"] == 1
    assert _rel(out["y"], free["y"]) < 1e-12 and _rel(out["dE"], free["dE"]) < 1e-12 and _rel(out["u"], free["u"]) < 1e-12
    fs.th.release_device()


def _mixed_rank(comm, krylov_first):
    """slot 0 direct and slot 1 factor-free on one partitioned handle, set up in either order: both solve to SuperLU's answer."""
    from flowcontrol_amd.device import SLOT_BDF2

    th, dev, dofs = _handle(comm)
    other = 1 - SLOT_BDF2
    x = th.node_coords
    U1 = np.r_[0.8 + 0.2 * np.cos(x[:, 1]), 0.1 * np.sin(x[:, 0])]
    dev.assemble_matrix(other, mass=1.0 / DT, nu=1.0 / RE, adv=U1, lin=U1)
    dev.apply_bc(other)
    steps = [lambda: dev.setup_krylov(SLOT_BDF2, sweeps=2, method="gmres", max_iter=300, rtol=1e-12), lambda: dev.setup_solver(other)]
    for s in steps if krylov_first else steps[::-1]:
        s()
    _, b = _vectors(th.N, dofs)
    res = {}
    for slot in (SLOT_BDF2, other):
        if slot == other:
            dev.set_solver_options(refine=0, method="refine")
        else:
            dev.set_solver_options(refine=300, method="gmres", rtol=1e-12)
        res[slot] = dev.solve(slot, b)[0]
    res["b"] = b
    dev.close()
    return res


@pytest.mark.parametrize("krylov_first", [True, False])
def test_mixed_slots_on_one_partitioned_handle(krylov_first):
    from flowcontrol_amd.comm import run_threaded
    from flowcontrol_amd.device import SLOT_BDF2

    outs = run_threaded(2, _mixed_rank, krylov_first)
    th, dev, _ = _handle()  # the complete matrices (a rank holds complete rows only for its own rows and the root's)
    x = th.node_coords
    U1 = np.r_[0.8 + 0.2 * np.cos(x[:, 1]), 0.1 * np.sin(x[:, 0])]
    dev.assemble_matrix(1 - SLOT_BDF2, mass=1.0 / DT, nu=1.0 / RE, adv=U1, lin=U1)
    dev.apply_bc(1 - SLOT_BDF2)
    for slot in (SLOT_BDF2, 1 - SLOT_BDF2):
        ref = spla.splu(dev.matrix(slot).tocsc()).solve(outs[0]["b"])
        for o in outs:
            assert _rel(o[slot], ref) <= 1e-10, (slot, _rel(o[slot], ref))
    dev.close()


def _open_loop_rank(comm, n):
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")
    fs = _solver(n, True)
    fs.comm = comm
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    for _ in range(n):
        fs.step([0.0, 0.0])
        assert fs.solve_info[1] < 1e-9
    ts = fs.timeseries
    out = {"y": ts[["y_meas_1", "y_meas_2", "y_meas_3"]].to_numpy(), "dE": ts["dE"].to_numpy()}
    fs.th.release_device()
    return out


def test_factor_free_open_loop_steps_on_two_ranks_follow_the_oracle():
    """The 50-step open-loop scenario of test_factor_free_time_steps_follow_the_oracle at world 2, against the golden series."""
    from flowcontrol_amd.comm import run_threaded

    n = 50
    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")
    for o in run_threaded(2, _open_loop_rank, n):
        assert _rel(o["y"], g["ol_y"][: n + 1]) <= 1e-8 and _rel(o["dE"], g["ol_dE"][: n + 1]) <= 1e-8


def _cn_rank(comm, nsteps):
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")
    fs = _solver(nsteps, True)
    fs.comm = comm
    fs.params_solver.time_scheme = "cn"
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    for k in range(nsteps):
        fs.step(np.array([0.05 * np.sin(0.4 * k), -0.03]))
    out = {"y": fs.timeseries[["y_meas_1", "y_meas_2", "y_meas_3"]].to_numpy()[1:], "u": fs.fields.u_.vector().get_local()}
    fs.th.release_device()
    return out


def test_factor_free_crank_nicolson_on_two_ranks_follows_the_oracle():
    """time_scheme="cn" (an operator in the right-hand side, fc_update_operator on the factor-free slot) at world 2 against the CPU
    oracle's Crank-Nicolson stepper, as test_factor_free_crank_nicolson_steps_follow_the_oracle does on one GPU."""
    from flowcontrol_amd.comm import run_threaded
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC
    from oracle import ns_oracle as O

    nsteps = 8
    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")
    outs = run_threaded(2, _cn_rank, nsteps)
    fs = _solver(nsteps, True)
    th = fs.th
    dofs, prof = fs._bc_tables()
    ts = O.TimeStepperCN(O.Disc.from_taylor_hood(th), 100.0, 0.005, g["UP0"][: 2 * th.nn], dofs, prof)
    rows = [s.row(fs) for s in fs.params_control.sensor_list]
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    u_n = fs.fields.ic.u.vector().get_local()
    ys = []
    for k in range(nsteps):
        up = ts.step(u_n, np.array([0.05 * np.sin(0.4 * k), -0.03]))
        u_n = up[: 2 * th.nn]
        ys.append([w @ up[i] for i, w in rows])
    for o in outs:
        assert _rel(o["y"], ys) <= 1e-8 and _rel(o["u"], u_n) <= 1e-8
    fs.th.release_device()


# ── other configurations: the pressure pin, a refined mesh at world 8, a body-force actuator ──
def _lidcavity(comm, nsteps, krylov):
    from flowcontrol_amd.examples.lidcavity.lidcavityflowsolver import LidCavityFlowSolver
    from flowcontrol_amd.fem.spaces import Function

    g = np.load(ROOT / "tests" / "golden" / "lidcavity_mesh64.npz")
    fs = LidCavityFlowSolver.make_default(Re=1000, path_out=tempfile.mkdtemp(), num_steps=nsteps)
    if krylov:
        fs.krylov_precond, fs.krylov_method, fs.krylov_max_iter, fs.krylov_rtol = "schur_amg", "gmres", 300, 1e-11
    if comm is not None:
        fs.comm = comm
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    for _ in range(nsteps):
        fs.step(u_ctrl=[0.0] * fs.params_control.actuator_number)
        assert fs.solve_info[1] < 1e-9
    ts = fs.timeseries
    out = {"y": ts[[c for c in ts.columns if c.startswith("y_meas_")]].to_numpy(), "dE": ts["dE"].to_numpy(),
           "u": fs.fields.u_.vector().get_local()}
    fs.th.release_device()
    return out


def test_enclosed_flow_in_factor_free_mode_on_two_ranks():
    """Lid-driven cavity (the pressure pinned at one dof: the shift enters the replicated Schur complement on every rank) in factor-free
    mode, on one GPU and at world 2, within 1e-8 of the run with factors."""
    from flowcontrol_amd.comm import run_threaded

    nsteps = 4
    ref = _lidcavity(None, nsteps, False)
    one = _lidcavity(None, nsteps, True)
    outs = run_threaded(2, _lidcavity, nsteps, True)
    for o in [one] + outs:
        for k in ("y", "dE", "u"):
            assert _rel(o[k], ref[k]) <= 1e-8, (k, _rel(o[k], ref[k]))


def _config4_rank(comm, nsteps):
    from flowcontrol_amd.examples.cylinder.scenarios import config4_actuation

    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver, refined_cylinder_mesh
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1_refined1.npz")
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=nsteps, meshpath=refined_cylinder_mesh(1))
    fs.krylov_precond, fs.krylov_method, fs.krylov_max_iter, fs.krylov_rtol = "schur_amg", "gmres", 300, 1e-11
    fs.comm = comm
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    u = config4_actuation(nsteps)
    for k in range(nsteps):
        fs.step(u[k])
        assert fs.solve_info[1] < 1e-9
    ts = fs.timeseries
    out = {"y": ts[[c for c in ts.columns if c.startswith("y_meas_")]].to_numpy(), "dE": ts["dE"].to_numpy(),
           "part": fs.th.device().krylov_partition_info(1)}
    fs.th.release_device()
    return out


def test_factor_free_config4_on_eight_thread_ranks():
    """BASELINE config 4 (refined O1) at world 8 in factor-free mode: 12 steps against the oracle's fixture."""
    from flowcontrol_amd.comm import run_threaded

    nsteps = 12
    g = np.load(ROOT / "tests" / "golden" / "cylinder_O1_refined1.npz")
    for o in run_threaded(8, _config4_rank, nsteps):
        assert _rel(o["y"], g["y"][: nsteps + 1]) < 1e-8 and _rel(o["dE"], g["dE"][: nsteps + 1]) < 1e-8
        assert o["part"]["exchanges_per_apply"] == 1


def _cavity_rank(comm, nsteps):
    from flowcontrol_amd.examples.cavity.cavityflowsolver import CavityFlowSolver
    from flowcontrol_amd.fem.spaces import Function

    g = np.load(ROOT / "tests" / "golden" / "cavity_coarse.npz")
    fs = CavityFlowSolver.make_default(Re=7500, path_out=tempfile.mkdtemp(), num_steps=nsteps)
    fs.krylov_precond, fs.krylov_method, fs.krylov_max_iter, fs.krylov_rtol = "schur_amg", "gmres", 300, 1e-11
    fs.comm = comm
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    for _ in range(nsteps):
        fs.step([0.0])
        assert fs.solve_info[1] < 1e-9
    ts = fs.timeseries
    out = {"y": ts[[c for c in ts.columns if c.startswith("y_meas")]].to_numpy(), "dE": ts["dE"].to_numpy()}
    fs.th.release_device()
    return out


def test_factor_free_cavity_with_body_force_on_two_ranks():
    """The cavity case (FORCE actuator: the body force enters the element loop on each rank's cells) at world 2, 10 steps against
    the oracle's series, as test_factor_free_cavity_with_body_force_follows_the_oracle does on one GPU."""
    from flowcontrol_amd.comm import run_threaded

    nsteps = 10
    g = np.load(ROOT / "tests" / "golden" / "cavity_coarse.npz")
    for o in run_threaded(2, _cavity_rank, nsteps):
        assert _rel(o["y"], g["y"][: nsteps + 1]) <= 1e-8 and _rel(o["dE"], g["dE"][: nsteps + 1]) <= 1e-8


# ── the distributed apply against the host model (tests/support/precond_model.py), launch list by launch list ──
def _rank_model_apply(comm, n, sweeps_list):
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from tests.support import krylov_model as km
    from tests.support import precond_model as pm

    th = TaylorHood(Mesh.unit_square(n, n))
    dev = DeviceSolver(th)
    dev.join(comm.rank, comm.world, comm.bcast, comm.allreduce)
    dofs = km.wall_dofs(th)
    dev.set_bc(dofs, np.zeros((dofs.size, 1)))
    dev.assemble_matrix(SLOT_BDF2, **pm.operator_args(th.node_coords))
    dev.apply_bc(SLOT_BDF2)
    out = {}
    for sweeps in sweeps_list:
        info = dev.setup_krylov(SLOT_BDF2, sweeps=sweeps, method="gmres", max_iter=60, rtol=1e-10)
        xs = pm.inputs(th.N, 2 * th.nn, dev.perm)
        ys = {k: dev.debug_apply_pc(SLOT_BDF2, x) for k, x in xs.items()}
        route = dev.pc_route(SLOT_BDF2)
        again = dev.debug_apply_pc(SLOT_BDF2, xs["random"])
        out[sweeps] = dict(info=info, part=dev.krylov_partition_info(SLOT_BDF2), apply=ys, again=again, route=route)
    out.update(perm=dev.perm.copy(), rowkind=dev.part.rowkind.copy(), rank=comm.rank)
    dev.close()
    return out


@pytest.mark.parametrize("n", [12, 16])
def test_distributed_apply_against_the_host_model(n):
    """World 2 on thread ranks, unit_square(12) (no sparse AMG level: the exchange buffer is the dense solve's right-hand side itself) and
    unit_square(16) (one level: the V-cycle reads the first level's right-hand side in the exchange buffer), one and two Jacobi sweeps
    (one: K_F is D^-1, an entry per row -- fc_pc_csr<4>): the merged apply within the single-GPU test's tolerances of the np.longdouble
    model built from the complete matrix, and on every rank the launch list the model predicts from the rank's row kinds -- two fills,
    K_F, fc_pc_bshare, the V-cycle, fc_pc_final_share."""
    from flowcontrol_amd.comm import run_threaded
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from tests.support import krylov_model as km
    from tests.support import precond_model as pm

    assert n in pm.SHARE_CASES
    outs = run_threaded(2, _rank_model_apply, n, pm.SHARE_SWEEPS)
    th = TaylorHood(Mesh.unit_square(n, n))
    dev = DeviceSolver(th)  # the complete matrix (a rank holds complete rows only for its own rows and the root's)
    dofs = km.wall_dofs(th)
    dev.set_bc(dofs, np.zeros((dofs.size, 1)))
    dev.assemble_matrix(SLOT_BDF2, **pm.operator_args(th.node_coords))
    dev.apply_bc(SLOT_BDF2)
    A = dev.matrix(SLOT_BDF2)
    dev.close()
    env = os.environ.get("FC_PC_AMG_SWEEPS")
    amg = max(1, min(2, int(env))) if env else 2  # (the library's default below 16 384 pressure dofs)
    n_vel, perm = 2 * th.nn, outs[0]["perm"]
    spec = pm.Spec(A, perm, n_vel)
    assert (th.N, spec.np, len(spec.levels)) == pm.CASES[n][:3]
    tol = pm.tolerances()
    xs = pm.inputs(th.N, n_vel, perm)
    lanes_seen = set()
    for sweeps in pm.SHARE_SWEEPS:
        refs = {k: spec.apply(x, sweeps, amg) for k, x in xs.items()}
        for o in outs:
            assert np.array_equal(o["perm"], perm)
            r = o[sweeps]
            assert abs(r["info"]["jacobi_omega"] - spec.omega(sweeps)) <= 1e-14 * spec.omega(sweeps)
            assert (r["info"]["amg_levels"], r["info"]["coarsest_rows"], r["info"]["pressure_dofs"]) == (len(spec.levels) + 1, spec.Ac.shape[0], spec.np)
            want = spec.share_route(o["rowkind"], o["rank"] == 0, sweeps, amg)
            assert np.array_equal(r["route"], want), f"route not taken: rank {o['rank']} sweeps {sweeps}: predicted {want.tolist()}, reported {r['route'].tolist()}"
            assert len(want) == r["info"]["launches_per_apply"]
            assert want[2][1] == r["part"]["velocity_rows"] and want[-1][1] == r["part"]["velocity_rows"] + r["part"]["pressure_rows"]
            lanes_seen |= {(int(k), int(ln)) for k, _, ln, _ in want}
            worst = 0.0
            for name in xs:
                errs = pm.part_errors(r["apply"][name], refs[name], n_vel)
                for e, t in zip(errs, tol):
                    for ev, tv in zip(e, t):
                        worst = max(worst, ev / tv)
                        assert ev <= tv, f"rank {o['rank']} sweeps {sweeps} {name}: the merged apply misses the longdouble model by {ev:.3e}, allowed {tv:.3e}"
                assert np.array_equal(r["apply"][name], outs[0][sweeps]["apply"][name]), "the ranks return different merged vectors"
            assert np.array_equal(r["again"], r["apply"]["random"]), "a after b differs from a"
            print(f"unit_square({n}) rank {o['rank']} sweeps {sweeps}: route {[(pm.KERNELS[k], nr, ln, lv) for k, nr, ln, lv in want.tolist()]}, worst {worst:.3f} x tolerance")
    assert (pm.CSR, 4) in lanes_seen, "fc_pc_csr<4> (K_F of one sweep: D^-1) was not predicted on any rank"
    assert {ln for k, ln in lanes_seen if k == pm.BSHARE} <= {4, 8}
