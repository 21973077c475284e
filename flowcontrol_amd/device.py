"""Host-side driver of one ``fc_handle``: numpy in, numpy out, everything else on the MI355X.

This is the only module that talks to ``libfc_hip.so``.  ``FlowSolver`` (the mirror of the
reference's ``src/flowcontrol/flowsolver.py``) owns one :class:`DeviceSolver`.
"""

from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS, SLOT_SCRATCH, check, ptr
from .fem.spaces import TaylorHood


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


logger = logging.getLogger(__name__)


class DeviceSolver:
    def __init__(self, th: TaylorHood, device: int = 0):
        self.lib = _lib.load()
        if _lib.device_count() <= 0:
            raise _lib.FcError(_lib.FC_ERR_HIP, "no HIP device visible: the MI355X path has no CPU fallback")
        self.th = th
        m = th.mesh
        self._h = C.c_void_p()
        check(
            self.lib.fc_create(
                C.byref(self._h), device, m.num_vertices, m.num_edges, m.num_cells, _f64(m.coords), _i32(m.cells), _i32(m.cell_edges)
            )
        )
        N, nnz, nn = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.fc_get_sizes(self._h, C.byref(N), C.byref(nnz), C.byref(nn)))
        self.N, self.nnz, self.nn = N.value, nnz.value, nn.value
        assert self.N == th.N and self.nn == th.nn
        self.rowptr = np.empty(self.N + 1, dtype=np.int32)
        self.colidx = np.empty(self.nnz, dtype=np.int32)
        check(self.lib.fc_get_pattern(self._h, self.rowptr, self.colidx))
        self.n_act = 0
        self.n_sens = 0
        self.perm: np.ndarray | None = None  # elimination ordering (new position -> W dof)
        self.factor_nnz: dict[int, int] = {}
        self.rank, self.world = 0, 1
        self.part = None  # multi-GPU: this rank's share (rowkind, local cells, exchange stages) as the library laid it out
        self._sensor_rows: list | None = None
        # the whole solver setup -- symbolic phase (tree, factor layout, elimination plan, sweep tables: csrc/fc_symbolic.hpp) and numeric
        # factorisation -- runs inside the library (fc_setup_solver).  The numpy specification the symbolic phase is compared with lives
        # with the tests (tests/support/ndsolver.py, tests/test_symbolic_cabi.py).
        self._tree_args = None
        self._structured: set[int] = set()
        self.refactor_ms: dict[int, float] = {}
        #: slot -> the factors missed the acceptance residual by the direct apply and serve as GMRES preconditioner (fc_accept_factors)
        self.factors_inexact: dict[int, bool] = {}
        self._probe: np.ndarray | None = None
        self._pin_shift = 1.0
        self._step_bufs = None
        self._ctrl_bank = None
        self._pin: int | None = None  # pressure dof of an enclosed flow whose level is fixed (diagonal shift in the factors)
        self._truncate = 0  # > 0: only the tree levels >= this are factorised (memory-lean preconditioner)
        self.device_index = device
        self.batch_k = 0
        self._batch_bufs = None
        self._xchg_error: BaseException | None = None

    # ── multi-GPU ────────────────────────────────────────────────────────────
    def join(self, rank: int, world: int, broadcast_bytes, host_allreduce=None, agree=None) -> None:
        """Make this handle rank ``rank`` of a ``world``-GPU run (one process per GPU).

        ``broadcast_bytes(b | None) -> bytes`` ships the 128-byte RCCL unique id from rank 0 to every
        rank (e.g. ``torch.distributed.broadcast_object_list``); the communicator then lives inside
        the library and its all-reduces run on the solver's own HIP stream.

        ``agree(flag: float) -> float`` (the max of ``flag`` over the ranks, through the caller's own process group): with it the
        ranks settle TOGETHER whether the RCCL communicator exists — every rank probes RCCL before the collective
        ``ncclCommInitRank`` and reports after it; on any failure every rank raises :class:`FcCommInitError` (a rank that did get a
        communicator gives it back first), so that all of them can take the host exchange instead of some waiting in a collective
        for a rank that never comes.
        """
        if world & (world - 1):
            raise ValueError("world size must be a power of two (one elimination sub-tree per GPU)")
        self.rank, self.world = int(rank), int(world)
        self._host_allreduce = host_allreduce
        # FC_FORCE_COMM=1 (test aid): build a 1-rank RCCL communicator and run the partitioned code
        # path (cell list, row kinds, in-stream all-reduces) on a single GPU
        self._force_comm = world == 1 and os.environ.get("FC_FORCE_COMM", "0") == "1"
        if world == 1 and not self._force_comm:
            return
        # another root for the elimination tree: whatever was set up for the single-GPU role is void
        self.perm, self.part = None, None
        self._structured.clear()
        if host_allreduce is not None:
            # exchange through the host (fc_set_host_exchange): no RCCL communicator; ``host_allreduce(array)`` sums a
            # float64 array over the ranks in place.  The launch sequence is the one of the RCCL path.
            def _cb(ptr, n, _user):
                # ctypes swallows an exception raised in a callback: park it, poison the buffer (the residual / divergence
                # checks of the step then trip instead of continuing on un-reduced sums) and re-raise after the C call
                arr = np.ctypeslib.as_array(ptr, shape=(int(n),))
                try:
                    host_allreduce(arr)
                except BaseException as err:  # noqa: BLE001
                    self._xchg_error = err
                    arr[:] = np.nan

            self._xchg_cb = _lib.EXCHANGE_FN(_cb)  # keep the callback object alive as long as the handle
            check(self.lib.fc_set_host_exchange(self._h, world, rank, C.cast(self._xchg_cb, C.c_void_p), None))
            self.comm_selftest()
            return
        import sys

        torch = sys.modules.get("torch")
        if world > 1 and torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized() \
                and torch.cuda.current_device() != self.device_index:
            # one process per GPU: RCCL would see duplicate devices if every rank's handle sat on GPU 0
            raise _lib.FcError(_lib.FC_ERR_INVALID, f"rank {rank}: the solver handle lives on GPU {self.device_index} but this process's "
                               f"current GPU is {torch.cuda.current_device()} (create the solver after torch.cuda.set_device(LOCAL_RANK))")
        # creating the communicator may fail for reasons of the machine (RCCL not loadable, ncclCommInitRank refused): that is
        # FcCommInitError, which a caller may answer with the host exchange; rank 0 ships an empty id instead of leaving the
        # others in the broadcast.  A communicator that exists but does not sum (comm_selftest) is a plain FcError: never retried
        if agree is not None:
            # before anything of RCCL is started (ncclGetUniqueId opens rank 0's bootstrap listener): can EVERY rank load RCCL?
            mine = None
            try:
                check(self.lib.fc_comm_probe(rank))
            except _lib.FcError as err:
                mine = err
            if agree(0.0 if mine is None else 1.0) != 0.0:
                raise _lib.FcCommInitError(mine if mine is not None else "another rank cannot load RCCL")
        buf = C.create_string_buffer(128)
        payload, first = None, None
        if rank == 0:
            try:
                check(self.lib.fc_comm_unique_id(buf))
                payload = buf.raw
            except _lib.FcError as err:
                payload, first = b"", err
        uid = broadcast_bytes(payload)
        if not uid:
            raise _lib.FcCommInitError(first if first is not None else "rank 0 could not create the RCCL unique id")
        mine = None
        try:
            check(self.lib.fc_comm_init(self._h, world, rank, C.create_string_buffer(uid, 128)))
        except _lib.FcError as err:
            mine = err
        if agree is not None and agree(0.0 if mine is None else 1.0) != 0.0:
            if mine is None:
                check(self.lib.fc_comm_destroy(self._h))  # mixed outcome: give the communicator back, everybody falls back
            raise _lib.FcCommInitError(mine if mine is not None else "another rank could not create its RCCL communicator")
        if mine is not None:
            raise _lib.FcCommInitError(mine) from mine
        self.comm_selftest()

    def comm_selftest(self) -> float:
        """Pre-flight of the exchange (``fc_comm_selftest``, every rank): one all-reduce of a known vector through the path
        the time steps use, checked on this rank; raises :class:`FcError` naming the first wrong entry."""
        err = C.c_double()
        code = self.lib.fc_comm_selftest(self._h, C.byref(err))
        self._raise_exchange_error()
        check(code)
        return err.value

    def comm_info(self) -> dict:
        """Ranks / rank / transport of the handle's exchange as the library sees it (RCCL: read back from the communicator)."""
        n, r, t = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.lib.fc_comm_info(self._h, C.byref(n), C.byref(r), C.byref(t)))
        return {"nranks": n.value, "rank": r.value, "transport": {0: "none", 1: "rccl", 2: "host"}[t.value]}

    def _raise_exchange_error(self) -> None:
        """An exception inside the host exchange callback (gloo timeout, dead peer) surfaces here, after the C call returned."""
        err, self._xchg_error = self._xchg_error, None
        if err is not None:
            raise _lib.FcError(_lib.FC_ERR_HIP, f"host exchange failed: {err!r}") from err

    # ── lifetime ─────────────────────────────────────────────────────────────
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.fc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ── matrices ─────────────────────────────────────────────────────────────
    def assemble_matrix(self, slot, mass=0.0, nu=0.0, adv=None, lin=None, adv_scale=1.0, lin_scale=1.0, pressure=-1.0, divergence=-1.0):
        adv = None if adv is None else _f64(adv)
        lin = None if lin is None else _f64(lin)
        check(self.lib.fc_assemble_matrix(self._h, slot, mass, nu, ptr(adv), adv_scale, ptr(lin), lin_scale, pressure, divergence))

    def matrix(self, slot) -> sp.csr_matrix:
        vals = np.empty(self.nnz)
        check(self.lib.fc_get_matrix_values(self._h, slot, vals))
        return sp.csr_matrix((vals, self.colidx.copy(), self.rowptr.copy()), shape=(self.N, self.N))

    def set_matrix_values(self, slot, vals) -> None:
        check(self.lib.fc_set_matrix_values(self._h, slot, _f64(vals)))

    def spmv(self, slot, x) -> np.ndarray:
        y = np.empty(self.N)
        check(self.lib.fc_spmv(self._h, slot, _f64(x), y))
        return y

    def bench_spmv(self, slot, reps=1000) -> float:
        ms = C.c_double()
        check(self.lib.fc_bench_spmv(self._h, slot, reps, C.byref(ms)))
        return ms.value

    # ── problem data ─────────────────────────────────────────────────────────
    def set_bc(self, bc_dofs, profiles) -> None:
        bc_dofs = _i32(bc_dofs)
        if len(bc_dofs) and np.size(profiles) == 0:  # Dirichlet dofs without an actuator (reshape cannot infer a width of 0)
            profiles = np.zeros((len(bc_dofs), 0))
        else:
            profiles = _f64(profiles).reshape(len(bc_dofs), -1) if len(bc_dofs) else np.zeros((0, np.shape(profiles)[-1] if np.ndim(profiles) > 1 else 0))
        self.n_act = profiles.shape[1]
        if self.perm is not None and not np.array_equal(np.sort(bc_dofs), np.sort(getattr(self, "bc_dofs", bc_dofs))):
            # the elimination tree parks the Dirichlet dofs in the leaves: a different set needs a new tree
            self.perm = None
            self._structured.clear()
        self.bc_dofs = bc_dofs
        check(self.lib.fc_set_bc(self._h, len(bc_dofs), ptr(bc_dofs), self.n_act, ptr(np.ascontiguousarray(profiles))))

    def set_force(self, profiles) -> None:
        if profiles is None:
            check(self.lib.fc_set_force(self._h, 0, None))
            return
        profiles = _f64(profiles).reshape(self.n_act, 2 * self.nn)
        check(self.lib.fc_set_force(self._h, self.n_act, ptr(profiles)))

    def set_sensors(self, rows: list[tuple[np.ndarray, np.ndarray]]) -> None:
        self._sensor_rows = rows  # (partitioned handles: the library restricts every row to the dofs this rank accounts for)
        self.n_sens = len(rows)
        rp = np.zeros(len(rows) + 1, dtype=np.int32)
        for i, (idx, _) in enumerate(rows):
            rp[i + 1] = rp[i] + len(idx)
        idx = _i32(np.concatenate([r[0] for r in rows])) if rows else np.zeros(0, np.int32)
        w = _f64(np.concatenate([r[1] for r in rows])) if rows else np.zeros(0)
        check(self.lib.fc_set_sensors(self._h, len(rows), ptr(rp), ptr(idx), ptr(w)))

    def set_time_scheme(self, dt: float, nonlinear: bool = True) -> None:
        check(self.lib.fc_set_time_scheme(self._h, float(dt), int(bool(nonlinear))))

    def apply_bc(self, slot) -> None:
        check(self.lib.fc_apply_bc(self._h, slot))

    # ── solver setup (analysis + factorisation inside the library) ───────────
    def setup_solver(self, slot: int, depth: int | None = None, refine: int = 0, check_residual: bool | int = True, merge: int = 2,
                     restructure: bool = False, truncate: int = 0) -> None:
        """Factorise the (BC-eliminated) matrix of ``slot`` on the device (``fc_setup_solver``).

        ``depth`` binary bisections (default: leaves of ≈ 12 cells), fused ``merge`` at a time into a
        2**merge-ary elimination tree (on ``world`` GPUs the root is ``world``-ary first: one sub-tree
        per rank); ``refine`` iterative-refinement sweeps per solve (the fp64 selected inverse is
        accurate to round-off on its own, so 0 + residual monitoring is the default).

        Tree, permutation, factor layout, elimination plan and sweep tables are laid out once per tree by the library's own
        symbolic phase (``csrc/fc_symbolic.hpp``); a later call for the same slot is just the numeric phase on the device
        (on a partitioned handle every rank factorises its own sub-tree and the root).

        ``truncate = d > 0`` (memory-lean preconditioner): only the tree levels ≥ d are factorised and stored (the
        sub-domain solves and their couplings to the separators above — memory shrinks towards O(nnz) as d grows); the
        Schur complement on the top d levels is replaced by a diagonal estimate.  The slot is then a PRECONDITIONER:
        solves and time steps go through GMRES / BiCGStab (``set_solver_options(method=...)``)."""
        if os.environ.get("FC_ND_DEPTH"):  # tuning aids: tree shape (binary bisections, levels fused per tree level)
            depth = int(os.environ["FC_ND_DEPTH"])
        if os.environ.get("FC_ND_MERGE"):
            merge = int(os.environ["FC_ND_MERGE"])
        self._setup_solver_native(slot, depth, refine, check_residual, merge, truncate)

    def _setup_solver_native(self, slot, depth, refine, check_residual, merge, truncate) -> None:
        """``fc_setup_solver``: tree, factor layout, elimination plan, sweep tables, numeric factorisation and its
        acceptance solve all happen inside the library; only sizes come back."""
        code = self.lib.fc_setup_solver(self._h, slot, int(depth or 0), int(merge), int(truncate), int(refine), int(check_residual))
        self._raise_exchange_error()
        check(code)
        info = np.zeros(10, dtype=np.int64)
        check(self.lib.fc_get_solver_info(self._h, slot, info))
        self._n_factor_values, self.total_factor_nnz, self.local_factor_nnz = int(info[0]), int(info[1]), int(info[2])
        self.factor_nnz[slot] = int(info[0])
        self.n_stages, self.depth = int(info[3]), int(info[4])
        self._truncate = int(truncate)
        if self.perm is None:
            self.perm = np.empty(self.N, dtype=np.int32)
            check(self.lib.fc_get_permutation(self._h, self.perm))
            self._tree_args = (int(depth or 0), int(merge))
        if (self.world > 1 or getattr(self, "_force_comm", False)) and self.part is None:
            from types import SimpleNamespace

            kind = np.empty(self.N, dtype=np.uint8)
            check(self.lib.fc_get_rowkind(self._h, kind))
            cells = np.empty(int(info[8]), dtype=np.int32)
            check(self.lib.fc_get_local_cells(self._h, cells))
            self.part = SimpleNamespace(rowkind=kind, local_cells=cells, ar_n=int(info[5]), ar_stage=int(info[6]), ar2_stage=int(info[7]))
        ms = C.c_double()
        check(self.lib.fc_get_refactor_ms(self._h, slot, C.byref(ms)))
        self.refactor_ms[slot] = ms.value
        flag = C.c_int32()
        check(self.lib.fc_get_factors_inexact(self._h, slot, C.byref(flag)))
        self.factors_inexact[slot] = bool(flag.value)
        if flag.value:
            logger.warning("slot %d: the direct factor apply misses 1e-10 on this operator; its solves run GMRES preconditioned by the factors", slot)
        self._structured.add(slot)
        self._solver_opts = (int(refine), int(check_residual), "refine", 1e-10)

    def set_factor_precision(self, bits: int) -> None:
        """Storage width of the factor values of every slot set up from now on: 64 = exact selected inverse (default), 32 / 16
        = compressed factors (fp32 / bfloat16, 50 % / 25 % of the memory; a preconditioner for ``method="gmres" | "bicgstab"``)."""
        if int(bits) != getattr(self, "_factor_bits", 64):
            self._structured.clear()
        check(self.lib.fc_set_factor_precision(self._h, int(bits)))
        self._factor_bits = int(bits)

    def factor_storage(self, slot: int) -> tuple[int, int]:
        """(bits per factor value, bytes of factor values held) of ``slot``."""
        bits, nbytes = C.c_int32(), C.c_int64()
        check(self.lib.fc_get_factor_storage(self._h, slot, C.byref(bits), C.byref(nbytes)))
        return bits.value, nbytes.value

    def set_pressure_pin(self, dof: int | None, shift: float = 1.0) -> None:
        """Enclosed flows (velocity prescribed on the whole boundary): the monolithic matrix is singular, the
        pressure being defined up to a constant.  A positive shift on the diagonal of ONE pressure dof inside
        the factorisation (the matrix itself has no pressure-pressure entries) selects, for every compatible
        right-hand side, exactly the solution with that pressure = 0 — nothing else changes."""
        dof = None if dof is None else int(dof)
        if dof is not None and not 2 * self.nn <= dof < self.N:
            raise ValueError("the pinned dof must be a pressure dof")
        if dof != self._pin:
            self._pin, self._pin_shift = dof, float(shift)
            self._probe = None
            check(self.lib.fc_set_pressure_pin(self._h, -1 if dof is None else dof, float(shift)))

    def refactor(self, slot: int) -> float:
        """Numeric factorisation of the slot's current matrix on the device (the structure of the first
        ``setup_solver`` is reused): what ``solver.set_operator(A)`` costs.  Returns device milliseconds."""
        if slot not in self._structured:
            raise RuntimeError("setup_solver(slot) must run once before refactor(slot)")
        if getattr(self, "_truncate", 0):
            # truncated factors (a preconditioner): the library redoes the numeric phase AND the diagonal stand-in of the dropped
            # levels' Schur complement in one call; the caller's Krylov options stay
            opts = self._solver_opts
            depth, merge = self._tree_args
            self._setup_solver_native(slot, depth, 0, opts[1], merge, self._truncate)
            self.set_solver_options(*opts)
            return self.refactor_ms[slot]
        ms = C.c_double()
        code = self.lib.fc_refactor(self._h, slot, C.byref(ms))
        self._raise_exchange_error()
        check(code)
        self.refactor_ms[slot] = ms.value
        # end-to-end acceptance of the new factors: one solve with a fixed right-hand side, residual
        # against the matrix itself (block-local pivoting in fc_fe_pivot is not trusted blindly)
        if self._probe is None:
            self._probe = np.cos(0.37 * np.arange(self.N) + 0.1)
            if self._pin is not None:
                self._probe[2 * self.nn :] = 0.0  # compatible with the constant-pressure null space
        # (on a partitioned handle the probe is a collective: every rank refactorises, every rank probes)
        res, inexact = C.c_double(), C.c_int32()
        code = self.lib.fc_accept_factors(self._h, slot, C.byref(res), C.byref(inexact))
        self._raise_exchange_error()
        check(code)
        self.factors_inexact[slot] = bool(inexact.value)
        if inexact.value:
            logger.warning("slot %d: the direct factor apply reaches only %.1e on this operator; its solves run GMRES preconditioned by the factors", slot, res.value)
        return ms.value

    def refactor_flops(self) -> tuple[float, float]:
        """Trailing-update flops of the last numeric factorisation: (as run, with every row of a multi-GPU root front swept)."""
        a, b = C.c_double(), C.c_double()
        check(self.lib.fc_get_refactor_flops(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def refactor_step_widths(self) -> np.ndarray:
        """Pivot columns per block step (32 / 64 / 128; 0: no fronts) that every level of the elimination plan took in the last
        numeric factorisation, deepest level first (``fc_get_refactor_steps``): which front kernels ran."""
        out = np.full(64, -1, dtype=np.int32)  # (a tree of 2**64 nodes does not exist: 64 levels always suffice)
        check(self.lib.fc_get_refactor_steps(self._h, out.size, out))
        return out[out >= 0].copy()

    def factor_values(self, slot: int) -> np.ndarray:
        """Factor values of ``slot`` as they sit on the device (the layout ``fcsym::layout_factors`` / ``tests/support/ndsolver.BlockFactors`` describe)."""
        n = int(self._n_factor_values)
        out = np.empty(n)
        check(self.lib.fc_get_factor_values(self._h, slot, n, out))
        return out

    def set_solver_options(self, refine: int = 0, check_residual: bool | int = True, method: str = "refine", rtol: float = 1e-10) -> None:
        """``check_residual``: 0 / False = no residual monitor, n >= 1 = the time steps form ``|b - A x| / |b|`` on every n-th step
        (``info[1]``; NaN on the steps in between).
        ``method="refine"``: factor sweeps (+ ``refine`` iterative-refinement sweeps) — what the time steps use.
        ``method="bicgstab"`` / ``"gmres"``: right-preconditioned BiCGStab / restarted GMRES(30), device-resident
        (``refine`` = iteration cap, ``rtol`` = relative residual target), with the slot's current factors as
        preconditioner; for :meth:`solve` only."""
        self._solver_opts = (int(refine), int(check_residual), method, float(rtol))
        m = {"refine": _lib.METHOD_REFINE, "bicgstab": _lib.METHOD_BICGSTAB, "gmres": _lib.METHOD_GMRES}[method]
        check(self.lib.fc_set_solver_options(self._h, m, int(refine), float(rtol), int(check_residual)))

    def setup_krylov(self, slot: int, sweeps: int = 2, method: str = "gmres", max_iter: int = 200, rtol: float = 1e-10,
                     check_residual: bool | int = True) -> dict:
        """Factorisation-free solver setup of ``slot`` (``fc_setup_krylov``): nothing is factorised; solves and time steps run
        the device GMRES / BiCGStab right-preconditioned by the SIMPLE / AMG block preconditioner (``sweeps`` damped-Jacobi
        sweeps on the velocity block, one smoothed-aggregation V-cycle on the pressure Schur complement ``B diag(F)^-1 Bt``).
        Memory O(nnz).  Returns the sizes of what was built (``krylov_info``).
        On a partitioned handle (``join``) this is a collective: every rank calls it; each computes its own rows and the root's, one
        exchange per preconditioner apply (``krylov_partition_info``)."""
        m = {"bicgstab": _lib.METHOD_BICGSTAB, "gmres": _lib.METHOD_GMRES}[method]
        code = self.lib.fc_setup_krylov(self._h, slot, int(sweeps), m, int(max_iter), float(rtol), int(check_residual))
        self._raise_exchange_error()
        check(code)
        self._structured.discard(slot)
        self._krylov_slots = getattr(self, "_krylov_slots", set()) | {slot}
        self._solver_opts = (int(max_iter), int(check_residual), method, float(rtol))
        if self.perm is None:
            self.perm = np.empty(self.N, dtype=np.int32)
            check(self.lib.fc_get_permutation(self._h, self.perm))
        if (self.world > 1 or getattr(self, "_force_comm", False)) and self.part is None:
            from types import SimpleNamespace

            kind = np.empty(self.N, dtype=np.uint8)
            check(self.lib.fc_get_rowkind(self._h, kind))
            cells = np.empty(self.partition_info()["rhs_cells"], dtype=np.int32)
            check(self.lib.fc_get_local_cells(self._h, cells))
            pinfo = self.krylov_partition_info(slot)
            self.part = SimpleNamespace(rowkind=kind, local_cells=cells, ar_n=pinfo["root_rows"], ar_stage=-1, ar2_stage=-1)
        self.factor_nnz[slot] = 0
        return self.krylov_info(slot)

    def krylov_partition_info(self, slot: int) -> dict:
        """This rank's share of the factor-free slot ``slot`` (``fc_get_krylov_partition_info``): the rows it computes, the exchanges
        of a preconditioner apply and what it holds on the device, rank-local and replicated."""
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_get_krylov_partition_info(self._h, slot, info))
        return {"velocity_rows": int(info[0]), "pressure_rows": int(info[1]), "root_rows": int(info[2]), "exchanges_per_apply": int(info[3]),
                "doubles_per_apply": int(info[4]), "local_bytes": int(info[5]), "replicated_bytes": int(info[6]),
                "exchanges_last_step": int(info[7])}

    def debug_apply_pc(self, slot: int, x: np.ndarray) -> np.ndarray:
        """M^-1 x with the factor-free preconditioner of ``slot`` (W layout; a collective on a partitioned handle: merged result)."""
        out = np.empty(self.N)
        code = self.lib.fc_debug_apply_pc(self._h, slot, _f64(x), out)
        self._raise_exchange_error()
        check(code)
        return out

    PC_KERNELS = ("csr", "dense", "final", "bshare", "final_share", "fill")
    PC_ROUTE_COLS = ("kernel", "rows", "lanes", "level")

    def pc_route(self, slot: int) -> np.ndarray:
        """What the last apply of the factor-free preconditioner of ``slot`` launched (``fc_get_pc_route``): one int32 row
        :attr:`PC_ROUTE_COLS` per launch, in launch order -- kernel (index into :attr:`PC_KERNELS`), rows, lanes per row, AMG level
        or -1.  Written by the launch sites themselves: which kernels ran."""
        out = np.zeros(1 + len(self.PC_ROUTE_COLS) * 48, dtype=np.int32)
        check(self.lib.fc_get_pc_route(self._h, slot, ptr(out), out.size))
        return out[1 : 1 + len(self.PC_ROUTE_COLS) * int(out[0])].reshape(-1, len(self.PC_ROUTE_COLS)).copy()

    def tree_info(self, min_tree: bool = False) -> dict:
        """Bisections fused per level of the elimination tree (root first) and, on request, the factor values of the
        all-binary-pairs tree of the same depth (``fc_get_tree_info``)."""
        bits, n = np.zeros(16, dtype=np.int32), C.c_int32()
        nnz = C.c_int64(-1)
        check(self.lib.fc_get_tree_info(self._h, bits, C.byref(n), C.cast(C.byref(nnz), C.c_void_p) if min_tree else None))
        return {"bits": [int(b) for b in bits[: n.value]], "nnz_min_tree": int(nnz.value) if min_tree else None}

    def krylov_info(self, slot: int) -> dict:
        """What ``setup_krylov`` holds on the device for ``slot``."""
        info, om = np.zeros(8, dtype=np.int64), C.c_double()
        check(self.lib.fc_get_krylov_info(self._h, slot, info, C.byref(om)))
        return {"bytes": int(info[0]), "velocity_dofs": int(info[1]), "pressure_dofs": int(info[2]), "amg_levels": int(info[3]),
                "coarsest_rows": int(info[4]), "launches_per_apply": int(info[5]), "jacobi_sweeps": int(info[6]),
                "setup_ms": int(info[7]), "jacobi_omega": om.value}

    def update_operator(self, slot: int) -> None:
        """The slot's matrix changed (assemble + apply_bc) but its factors are kept: refresh the permuted copy
        only.  ``solve`` with ``method="bicgstab"`` then uses the old factors as preconditioner."""
        if slot not in self._structured and slot not in getattr(self, "_krylov_slots", ()):
            raise RuntimeError("setup_solver(slot) must run once before update_operator(slot)")
        check(self.lib.fc_update_operator(self._h, slot))

    def _upload_energy_matrix(self) -> None:
        """(u, v) mass matrix in the permuted numbering for the fused energy evaluation."""
        self.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        M = self.matrix(SLOT_MASS)
        nn2 = 2 * self.nn
        M = sp.block_diag([M[:nn2, :nn2], sp.csr_matrix((self.N - nn2, self.N - nn2))]).tocsr()
        M.eliminate_zeros()
        p = self.perm
        Mp = M[p][:, p].tocsr()
        Mp.sort_indices()
        check(self.lib.fc_set_energy_matrix(self._h, _i32(Mp.indptr), _i32(Mp.indices), _f64(Mp.data)))

    # ── state ────────────────────────────────────────────────────────────────
    def set_state(self, u_n, u_nn, p_n=None) -> None:
        p = None if p_n is None else _f64(p_n)
        check(self.lib.fc_set_state(self._h, _f64(u_n), _f64(u_nn), ptr(p)))

    def partition_info(self) -> dict:
        """Cells this rank computes the right-hand side for / assembles element matrices of, lead flag, ranks."""
        out = np.zeros(4, dtype=np.int32)
        check(self.lib.fc_get_partition_info(self._h, out))
        return {"rhs_cells": int(out[0]), "matrix_cells": int(out[1]), "lead": bool(out[2]), "ranks": int(out[3])}

    def undo_step(self) -> None:
        """``fc_undo_step``: (u_n, u_nn, p_n) as they were before the last single step (after FC_ERR_DIVERGED: the reference's
        state is untouched by a failed step, flowsolver.py:727-751)."""
        check(self.lib.fc_undo_step(self._h))

    def get_state(self):
        u_n, u_nn, p_n = np.empty(2 * self.nn), np.empty(2 * self.nn), np.empty(self.th.nv)
        check(self.lib.fc_get_state(self._h, ptr(u_n), ptr(u_nn), ptr(p_n)))
        return u_n, u_nn, p_n

    def owned_mask(self) -> np.ndarray:
        """W-layout mask of the dofs whose values this rank is responsible for when fields are merged."""
        if self.part is None:
            return np.ones(self.N, dtype=bool)
        k = self.part.rowkind
        return (k == 1) | ((k == 2) & (self.rank == 0))

    def get_solution(self) -> np.ndarray:
        up = np.empty(self.N)
        check(self.lib.fc_get_solution(self._h, up))
        return up

    # ── snapshot bank (fc_state_snap_*; flowcontrol_amd/modal.py) ───────────────────────────────
    def snap_reserve(self, capacity: int, every: int = 1, first: int = 0) -> None:
        """A new, empty snapshot bank of ``capacity`` columns per set (0 frees it): from now on the steps of this handle are counted and
        every ``every``-th one after the first ``first`` is gathered into set 0 by a launch of the step itself."""
        check(self.lib.fc_state_snap_reserve(self._h, int(capacity), int(every), int(first)))

    def snap_info(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_state_snap_info(self._h, info))
        return dict(zip(("capacity", "count", "kept", "every", "first", "steps", "dropped", "bytes"), (int(v) for v in info)))

    def snap_push(self) -> None:
        check(self.lib.fc_state_snap_push(self._h))

    def snap_load(self, set_: int, col0: int, X) -> None:
        X = _f64(X).reshape(-1, self.N)
        check(self.lib.fc_state_snap_load(self._h, int(set_), int(col0), X.shape[0], X))

    def snap_get(self, set_: int, col0: int, ncol: int) -> np.ndarray:
        out = np.empty((max(int(ncol), 0), self.N))
        check(self.lib.fc_state_snap_get(self._h, int(set_), int(col0), int(ncol), out))
        return out

    def snap_clear(self, set_: int) -> None:
        check(self.lib.fc_state_snap_clear(self._h, int(set_)))

    def snap_mean(self, set_: int, c0: int, c1: int, subtract: bool = False, download: bool = True) -> np.ndarray | None:
        out = np.empty(self.N) if download else None
        check(self.lib.fc_state_snap_mean(self._h, int(set_), int(c0), int(c1), int(bool(subtract)), ptr(out)))
        return out

    def snap_gram(self, lset: int, a0: int, a1: int, rset: int, b0: int, b1: int, weight_slot: int = -1) -> np.ndarray:
        """``L[:, a0:a1]^T Wt R[:, b0:b1]`` of the sets ``lset`` / ``rset``; ``weight_slot`` -1: identity, else the matrix in that slot."""
        out = np.empty((max(int(a1) - int(a0), 0), max(int(b1) - int(b0), 0)))
        check(self.lib.fc_state_snap_gram(self._h, int(lset), int(a0), int(a1), int(rset), int(b0), int(b1), int(weight_slot), out))
        return out

    def snap_gram_last(self) -> dict:
        """Device milliseconds (HIP events), algorithmic bytes and flops of the last :meth:`snap_gram`."""
        out = np.zeros(3)
        check(self.lib.fc_bench_state_snap_gram_last(self._h, out))
        return {"ms": float(out[0]), "bytes": float(out[1]), "flops": float(out[2])}

    def snap_combine(self, set_: int, c0: int, c1: int, Q, keep: bool = False, download: bool = True) -> np.ndarray | None:
        """``out[c] = sum_j Q[j, c] X_j`` over the columns ``[c0, c1)`` of a set; ``keep`` appends the vectors to set 1."""
        Q = _f64(Q).reshape(int(c1) - int(c0), -1)
        out = np.empty((Q.shape[1], self.N)) if download else None
        check(self.lib.fc_state_snap_combine(self._h, int(set_), int(c0), int(c1), Q.shape[1], Q, int(bool(keep)), ptr(out)))
        return out

    # ── hot path ─────────────────────────────────────────────────────────────
    def set_rhs_operator(self, slot: int, Cmat: sp.csr_matrix | None) -> None:
        """b -= C u_n with C given in W numbering (N × 2nn); rows are permuted here."""
        if Cmat is None:
            check(self.lib.fc_set_rhs_operator(self._h, slot, None, None, None))
            return
        Cp = Cmat.tocsr()[self.perm].tocsr()
        Cp.eliminate_zeros()
        Cp.sort_indices()
        check(self.lib.fc_set_rhs_operator(self._h, slot, ptr(_i32(Cp.indptr)), ptr(_i32(Cp.indices)), ptr(_f64(Cp.data))))

    def _step_buffers(self):
        # persistent argument buffers and their ctypes pointers: the call is on the critical path of
        # every synchronous step (a fresh ndarray + ctypes cast per argument costs ~1 us each)
        b = self._step_bufs
        if b is None or b[0].size != max(self.n_act, 1) or b[2].size != max(self.n_sens, 1):
            arrs = (np.zeros(max(self.n_act, 1)), np.zeros(max(self.n_act, 1)), np.empty(max(self.n_sens, 1)), np.empty(4))
            dE = C.c_double()
            b = self._step_bufs = arrs + (dE, tuple(ptr(a) for a in arrs), C.byref(dE))
        return b

    def step_begin(self, order_slot: int, u_ctrl, compute_energy: bool = True, u_force=None) -> None:
        """First half of :meth:`step`: hand the controls over and enqueue the step; the GPU works from here on."""
        u, uf, y, info, dE, (pu, puf, py, pinfo), pdE = self._step_buffers()
        if self.n_act:
            u[:] = u_ctrl
            if u_force is not None:
                uf[:] = u_force
        code = self.lib.fc_step_begin(self._h, order_slot, pu if self.n_act else None, puf if (self.n_act and u_force is not None) else None,
                                      1 if compute_energy else 0)
        if code:
            check(code)

    def step_end(self, early: bool = False):
        """Second half: wait for the step's record; returns (y, dE, info) like :meth:`step`.

        ``early=True``: return as soon as the measurements (and the non-finite flag) are there — ``(y, None, None)`` — and leave
        energy / solve info to :meth:`step_collect`; on a single-GPU handle they are computed on a second stream while the host and
        the next step go on (``fc_step_collect`` in fc_hip.h)."""
        u, uf, y, info, dE, (pu, puf, py, pinfo), pdE = self._step_bufs
        code = self.lib.fc_step_end(self._h, py, None if early else pdE, None if early else pinfo)
        if self._xchg_error is not None:
            self._raise_exchange_error()
        if code:
            check(code)
        if early:
            return y[: self.n_sens].copy(), None, None
        return y[: self.n_sens].copy(), dE.value, info

    def step_collect(self):
        """(dE, info) of the last step collected with ``step_end(early=True)``; blocks until they exist."""
        u, uf, y, info, dE, (pu, puf, py, pinfo), pdE = self._step_bufs
        check(self.lib.fc_step_collect(self._h, pdE, pinfo))
        return dE.value, info

    def step(self, order_slot: int, u_ctrl, compute_energy: bool = True, u_force=None):
        """One blocking ``fc_step``: (y, dE, info) of this step, all waited for."""
        u, uf, y, info, dE, (pu, puf, py, pinfo), pdE = self._step_buffers()
        if self.n_act:
            u[:] = u_ctrl
            if u_force is not None:
                uf[:] = u_force
        code = self.lib.fc_step(self._h, order_slot, pu if self.n_act else None, puf if (self.n_act and u_force is not None) else None, py, pdE,
                                1 if compute_energy else 0, pinfo)
        if self._xchg_error is not None:
            self._raise_exchange_error()
        if code:
            check(code)
        return y[: self.n_sens].copy(), dE.value, info

    def run(self, first_order_slot: int, n_steps: int, u_ctrl, compute_energy: bool = True):
        u = _f64(u_ctrl)
        is_seq = int(u.ndim == 2)
        y = np.empty((n_steps, max(self.n_sens, 1)))
        yv = np.empty((n_steps, self.n_sens))
        dE = np.empty(n_steps)
        check(self.lib.fc_run(self._h, first_order_slot, n_steps, ptr(u), is_seq, ptr(yv), ptr(dE), int(compute_energy)))
        del y
        return yv, dE

    # ── adjoint time stepping (csrc/fc_adjoint.hip.h; flowcontrol_amd/adjoint.py) ────────────
    def set_adjoint_factors(self, slot: int, on: int = 1) -> None:
        """``fc_set_adjoint_factors``: 1 builds the transposed factor and matrix values of ``slot`` (a second fp64 array each), 0 keeps
        them but refuses adjoint calls, -1 frees them (with the last slot: every buffer of the backward march)."""
        check(self.lib.fc_set_adjoint_factors(self._h, int(slot), int(on)))

    def adjoint_info(self, slot: int) -> dict:
        info, d = np.zeros(8, dtype=np.int64), np.zeros(2)
        check(self.lib.fc_adjoint_info(self._h, int(slot), ptr(info), ptr(d)))
        return {"available": bool(info[0]), "stale": bool(info[1]), "in_use": bool(info[2]), "slot_bytes": int(info[3]),
                "shared_bytes": int(info[4]), "bytes": int(info[3] + info[4]), "exports": int(info[5]), "export_ms": float(d[0]), "run_ms": float(d[1])}

    def adjoint_factor_values(self, slot: int) -> np.ndarray:
        """Transposed factor values of ``slot`` as they sit on the device, in the layout of :meth:`factor_values` (test aid)."""
        n = int(self.factor_nnz[slot])
        out = np.empty(n)
        check(self.lib.fc_debug_get_adjoint_factors(self._h, int(slot), n, out))
        return out

    def solve_transposed(self, slot: int, b):
        """``A_slot^T x = b`` on the transposed factors (``fc_solve_transposed``): ``(x, info)`` like :meth:`solve`."""
        x, info = np.empty(self.N), np.empty(4)
        check(self.lib.fc_solve_transposed(self._h, int(slot), _f64(b), x, ptr(info)))
        return x, info

    def run_adjoint(self, first_order_slot: int, n_steps: int, w=None, terminal=None, state_gradients: bool = True):
        """The backward march of a forward :meth:`run` of ``n_steps`` steps that started on ``first_order_slot``
        (``fc_run_adjoint``): for ``J = sum_m w[m - 1] . y_m + terminal . x_n`` returns ``(g [n, n_act], dx0 [N], dxm1 [N])``, the
        gradients with respect to the control sequence and the two initial time levels (W layout; ``None`` without
        ``state_gradients``)."""
        n = int(n_steps)
        wq = None if w is None else _f64(w).reshape(n, self.n_sens)
        z = None if terminal is None else _f64(terminal).reshape(self.N)
        g = np.zeros((n, self.n_act))
        dx0, dxm1 = (np.empty(self.N), np.empty(self.N)) if state_gradients else (None, None)
        check(self.lib.fc_run_adjoint(self._h, int(first_order_slot), n, ptr(wq), ptr(z), ptr(g), ptr(dx0), ptr(dxm1)))
        return g, dx0, dxm1

    def adjoint_reset(self, terminal=None) -> None:
        """Start a backward march step by step (``fc_adjoint_reset``): both adjoint levels zero, ``terminal`` added by the next step."""
        z = None if terminal is None else _f64(terminal).reshape(self.N)
        check(self.lib.fc_adjoint_reset(self._h, ptr(z)))

    def step_adjoint(self, slot: int, cm_n: float, cm_nn_next: float, w=None) -> np.ndarray:
        """One backward step on ``slot`` (``fc_step_adjoint``); returns ``dJ/du`` of that step, (n_act,)."""
        wq = None if w is None else _f64(w).reshape(self.n_sens)
        g = np.zeros(max(self.n_act, 1))
        check(self.lib.fc_step_adjoint(self._h, int(slot), float(cm_n), float(cm_nn_next), ptr(wq), ptr(g)))
        return g[: self.n_act]

    def adjoint_mass_product(self, cm_n: float, cm_nn: float) -> np.ndarray:
        """``M Z (cm_n mu_last + cm_nn mu_before)`` of the march so far, W layout (``fc_adjoint_mass_product``): the state gradients."""
        out = np.empty(self.N)
        check(self.lib.fc_adjoint_mass_product(self._h, float(cm_n), float(cm_nn), out))
        return out

    def adjoint_tape_reserve(self, capacity: int) -> None:
        """A state tape of ``capacity`` steps for the adjoint of the NONLINEAR stepper (``fc_adjoint_tape_reserve``; 0 frees it):
        ``capacity + 2`` columns of N doubles on the device, 8 N bytes per step.  Nothing is taped before :meth:`adjoint_tape_begin`."""
        check(self.lib.fc_adjoint_tape_reserve(self._h, int(capacity)))

    def adjoint_tape_begin(self) -> None:
        """Start taping at the present state (``fc_adjoint_tape_begin``): every step from here on appends its new state, until
        :meth:`set_state` or a new solver structure ends the tape.  :meth:`run_adjoint` then marches back over exactly that run."""
        check(self.lib.fc_adjoint_tape_begin(self._h))

    def adjoint_tape_info(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_adjoint_tape_info(self._h, info))
        out = {"capacity": int(info[0]), "count": int(info[1]), "overflowed": bool(info[2]), "bytes": int(info[3]), "begun": bool(info[4]),
               "lost": int(info[5])}
        if info[6] > 0:  # the checkpointed tape: its spacing and the forward steps the last march recomputed
            out["every"], out["replayed"] = int(info[6]), int(info[7])
        return out

    def adjoint_tape_reserve_sparse(self, capacity: int, every: int) -> None:
        """The CHECKPOINTED state tape (``fc_adjoint_tape_reserve_sparse``; ``every = 0`` or ``capacity = 0`` frees it): the pair of time
        levels in front of every ``every``-th step for the whole run, one dense segment of ``every`` steps and the controls every step
        read -- ``2 ceil(capacity / every) + every + 2`` columns of N doubles instead of ``capacity + 2``.  A march over it recomputes one
        segment at a time and returns the dense tape's gradients bit for bit.  Replaces a dense tape, and is replaced by one."""
        check(self.lib.fc_adjoint_tape_reserve_sparse(self._h, int(capacity), int(every)))

    def step_counts(self) -> tuple[int, int]:
        """``(single, batched)`` steps the handle has enqueued (``fc_debug_get_step_count``; test aid)."""
        single, batched = C.c_int64(0), C.c_int64(0)
        check(self.lib.fc_debug_get_step_count(self._h, C.byref(single), C.byref(batched)))
        return int(single.value), int(batched.value)

    def adjoint_segment_states(self) -> tuple[int, np.ndarray]:
        """``(j, X)``: the segment the checkpointed tape's buffer holds and its ``every + 2`` columns in the W layout -- row 0 is
        ``x_{j every - 1}``, row i + 1 is ``x_{j every + i}`` (test aid; rows beyond the run hold whatever an earlier segment left)."""
        ncol = self.adjoint_tape_info()["every"] + 2
        Xp = np.empty((ncol, self.N))
        seg = C.c_int32(0)
        check(self.lib.fc_debug_get_adjoint_segment(self._h, 0, ncol, Xp, C.byref(seg)))
        return int(seg.value), self._unpermuted_columns(Xp)

    def _unpermuted_columns(self, Xp: np.ndarray) -> np.ndarray:
        """Rows of N values in the solver's numbering -> the W layout (``self.perm`` is fetched once)."""
        if self.perm is None:
            self.perm = np.empty(self.N, dtype=np.int32)
            check(self.lib.fc_get_permutation(self._h, self.perm))
        X = np.empty_like(Xp)
        X[:, self.perm] = Xp
        return X

    def adjoint_tape_states(self) -> np.ndarray:
        """The taped states ``x_{-1}, x_0, x_1 .. x_count`` in the W layout, (count + 2, N) (test aid: the tape itself is kept in the
        solver's numbering)."""
        ncol = self.adjoint_tape_info()["count"] + 2
        Xp = np.empty((ncol, self.N))
        check(self.lib.fc_debug_get_adjoint_tape(self._h, 0, ncol, Xp))
        return self._unpermuted_columns(Xp)

    # ── tangent-linear march (csrc/fc_tangent.hip.h; flowcontrol_amd/tangent.py): Jacobian-vector products of a nonlinear run ────
    def tangent_reserve(self, on: int = 1) -> None:
        """``fc_tangent_reserve``: 1 allocates the tangent march's own buffers for the present mode (single, or the width of
        :meth:`set_batch`), 0 frees them.  A handle that never reserves allocates and launches nothing for the march."""
        check(self.lib.fc_tangent_reserve(self._h, int(on)))

    def tangent_info(self) -> dict:
        info, d = np.zeros(8, dtype=np.int64), np.zeros(2)
        check(self.lib.fc_tangent_info(self._h, ptr(info), ptr(d)))
        return {"reserved": bool(info[0]), "KB": int(info[1]), "bytes": int(info[2]), "steps": int(info[3]), "route": int(info[4]),
                "marches": int(info[5]), "run_ms": float(d[0])}

    def tangent_set_energy(self, on: int = 1) -> None:
        """``fc_tangent_set_energy``: with 1 every later tangent march of the handle also forms ``d(dE_m) = x_m^T M_s dx_m``, the
        directional derivative of the energy each forward step logs (one launch behind each step's tail, one fold behind the last
        step; :meth:`tangent_energy` returns the rows); 0 frees the rows.  :meth:`tangent_reserve` comes first, and the option goes
        with the reserve.  A linearised closed-loop march then needs the dense state tape of the run."""
        check(self.lib.fc_tangent_set_energy(self._h, int(on)))

    def tangent_energy_info(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_tangent_energy_info(self._h, info))
        return {"on": bool(info[0]), "have": bool(info[1]), "kernel": int(info[2]), "grid": int(info[3]), "steps": int(info[4]), "k": int(info[5]),
                "launches": int(info[6]), "bytes": int(info[7])}

    def tangent_energy(self) -> np.ndarray:
        """``d(dE_m)``, m = 1 .. n, of the last tangent march (``fc_get_tangent_energy``): (n,) after a single march, (n, k) after a
        batched one.  Raises if that march ran without :meth:`tangent_set_energy`."""
        info = self.tangent_energy_info()
        n, k = info["steps"], info["k"]
        dde = np.zeros((max(n, 1), k) if k else max(n, 1))
        check(self.lib.fc_get_tangent_energy(self._h, n, k, dde))
        return dde

    def tangent_tape_reserve(self, n_steps: int) -> None:
        """``fc_tangent_tape_reserve``: ``n_steps`` columns of N doubles in which every later single tangent march of at most
        ``n_steps`` steps keeps its states ``dx_1 .. dx_n`` (8 N bytes copied per step); 0 frees.  Single mode only.  What
        :meth:`set_adjoint_energy_source` reads."""
        check(self.lib.fc_tangent_tape_reserve(self._h, int(n_steps)))

    def tangent_tape_info(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_tangent_tape_info(self._h, info))
        return {"capacity": int(info[0]), "count": int(info[1]), "first_slot": int(info[2]), "bytes": int(info[3])}

    def tangent_tape_states(self) -> np.ndarray:
        """The tangent states ``dx_1 .. dx_count`` the tangent tape holds, in the W layout, (count, N) (test aid: the tape itself is
        kept in the solver's numbering)."""
        ncol = self.tangent_tape_info()["count"]
        Xp = np.empty((ncol, self.N))
        check(self.lib.fc_debug_get_tangent_tape(self._h, 0, ncol, Xp))
        return self._unpermuted_columns(Xp)

    def set_adjoint_energy_source(self, source: int = 0) -> None:
        """``fc_set_adjoint_energy_source``: 0 (the default) the weights of :meth:`set_adjoint_energy` multiply the taped states
        ``x_m``; 1 they multiply the tangent tape's ``dx_m`` in :meth:`run_adjoint` and :meth:`run_adjoint_closed_loop` -- the backward
        march of a Gauss-Newton product of the energy cost.  Falls back to 0 when the rows are cleared."""
        check(self.lib.fc_set_adjoint_energy_source(self._h, int(source)))

    #: entries of :meth:`tangent_route` (``FC_TAN_ROUTE_COLS`` of include/fc_hip_internal.h)
    TAN_ROUTE_COLS = ("elem", "g_elem", "g_gather", "KB", "k", "ref_col", "force_b", "fvec", "refined", "g_tail", "l1", "l2", "t2", "slot")

    def tangent_route(self) -> np.ndarray:
        """What the last tangent step of this handle launched, single or batched (``fc_get_tangent_route``): int32 entries
        :attr:`TAN_ROUTE_COLS`, written by the launch sites while they enqueue (test aid).  No launch, no synchronisation."""
        out = np.zeros(len(self.TAN_ROUTE_COLS), dtype=np.int32)
        check(self.lib.fc_get_tangent_route(self._h, out.size, ptr(out)))
        return out

    def tangent_stage(self) -> dict:
        """The buffers of the last tangent step as the march holds them, in the solver's PERMUTED numbering
        (``fc_debug_get_tangent_stage``, test aid): ``ev`` (12, nc) the element vectors, ``b`` the right-hand side, ``x`` / ``dx`` the
        solve's output (``dx`` None unless ``refined``), ``new`` the level the tail wrote, ``other`` the step's ``d1``, ``du`` / ``dy``
        the step's control and sensor rows, ``flags`` (32,), ``lift`` / ``fvec`` (n_act, N; ``fvec`` None without force vectors).  After
        a batched step the vectors are (N, KB), ``ev`` is (12, nc, KB), ``du`` (KB, n_act) and ``dy`` (k, n_sens).  Call it straight
        after the march: later calls of the handle reuse the buffers."""
        r = dict(zip(self.TAN_ROUTE_COLS, (int(v) for v in self.tangent_route())))
        kb = r["KB"]
        nc = int(self.th.mesh.cells.shape[0])
        shape = (self.N, kb) if kb else (self.N,)
        ev = np.empty((12, nc, kb) if kb else (12, nc))
        b, x, dx, new, other = (np.empty(shape) for _ in range(5))
        du = np.zeros((kb, self.n_act) if kb else (self.n_act,))
        dy = np.zeros((r["k"], self.n_sens) if kb else (self.n_sens,))
        flags = np.zeros(32, dtype=np.int32)
        lift, fvec = (np.zeros((self.n_act, self.N)) for _ in range(2))
        has_dx, has_f = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        check(self.lib.fc_debug_get_tangent_stage(self._h, kb, ptr(ev), ptr(b), ptr(x), ptr(dx), ptr(has_dx), ptr(new), ptr(other), ptr(du), ptr(dy),
                                                  ptr(flags), ptr(lift), ptr(fvec), ptr(has_f)))
        if self.perm is None:
            self.perm = np.empty(self.N, dtype=np.int32)
            check(self.lib.fc_get_permutation(self._h, self.perm))
        return {"ev": ev, "b": b, "x": x, "dx": dx if has_dx[0] else None, "refined": bool(has_dx[0]), "new": new, "other": other, "du": du, "dy": dy,
                "flags": flags, "lift": lift, "fvec": fvec if has_f[0] else None}

    def run_tangent(self, first_order_slot: int, n_steps: int, du=None, dx0=None, dxm1=None):
        """The tangent of the taped forward :meth:`run` of ``n_steps`` steps that started on ``first_order_slot`` (``fc_run_tangent``):
        the perturbation ``du [n, n_act]`` of the controls and ``dx0``, ``dxm1`` [N] (W layout; pressure rows are never read) of the two
        initial time levels (``None``: zero) stepped along the trajectory on the state tape.  Returns ``(dy [n, n_sens], dx_n [N],
        dx_{n-1} [N])``."""
        n = int(n_steps)
        duq = None if du is None else _f64(du).reshape(n, self.n_act)
        a = None if dx0 is None else _f64(dx0).reshape(self.N)
        b = None if dxm1 is None else _f64(dxm1).reshape(self.N)
        dy, dxn, dxnm1 = np.zeros((n, self.n_sens)), np.empty(self.N), np.empty(self.N)
        check(self.lib.fc_run_tangent(self._h, int(first_order_slot), n, ptr(duq), ptr(a), ptr(b), ptr(dy), ptr(dxn), ptr(dxnm1)))
        return dy, dxn, dxnm1

    def run_tangent_batch(self, first_order_slot: int, n_steps: int, du=None, dx0=None, dxm1=None, ref_col: int | None = None):
        """k tangent marches in lock step over the batched state tape (``fc_run_tangent_batch``): ``du [n, k, n_act]``, ``dx0`` /
        ``dxm1 [k, N]`` (``None``: zero) -> ``(dy [n, k, n_sens], dx_n [k, N], dx_{n-1} [k, N])``.  ``ref_col=None``: column s perturbs
        trajectory s; ``ref_col=c``: every column perturbs trajectory c.  A column that goes non-finite raises :class:`FcDiverged`;
        ``self.tangent_batch_flags`` (k,) then marks it and ``self.tangent_batch_last`` holds the arrays -- the others are valid."""
        n, k = int(n_steps), self.batch_k
        duq = None if du is None else _f64(du).reshape(n, k, self.n_act)
        a = None if dx0 is None else _f64(dx0).reshape(k, self.N)
        b = None if dxm1 is None else _f64(dxm1).reshape(k, self.N)
        dy, dxn, dxnm1 = np.zeros((n, k, self.n_sens)), np.empty((k, self.N)), np.empty((k, self.N))
        flags = self.tangent_batch_flags = np.zeros(max(k, 1), dtype=np.int32)
        self.tangent_batch_last = (dy, dxn, dxnm1)
        check(self.lib.fc_run_tangent_batch(self._h, int(first_order_slot), k, n, -1 if ref_col is None else int(ref_col), ptr(duq), ptr(a), ptr(b),
                                            ptr(dy), ptr(dxn), ptr(dxnm1), ptr(flags)))
        return dy, dxn, dxnm1

    # ── tangent of a closed loop (csrc/fc_tangent_loop.hip.h): Jacobian-vector products of the controller problem ────────────────
    #: keys of a closed-loop direction, in the order of the C ABI: those of :meth:`run_adjoint_closed_loop`'s gradients
    TAN_LOOP_KEYS = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u")

    def _tangent_loop_direction(self, direction, n: int, k: int | None):
        """The arrays of ``direction`` in the bank's shapes (leading k for a batch; signals ``(n, [k,] width)``); absent keys: None."""
        bank = self._ctrl_bank
        if bank is None:
            raise RuntimeError("set_controllers first")
        nx, nyc, nuc, ns, na = bank["nx"], bank["nyc"], bank["nuc"], self.n_sens, self.n_act
        shapes = {"Ad": (nx, nx), "Bd": (nx, nyc), "C": (nuc, nx), "D": (nuc, nyc), "G": (nyc, ns), "g0": (nyc,), "S": (na, nuc), "x0": (nx,), "y0": (ns,)}
        direction = dict(direction or {})
        unknown = set(direction) - set(self.TAN_LOOP_KEYS)
        if unknown:
            raise KeyError(f"closed-loop direction: unknown keys {sorted(unknown)} (known: {self.TAN_LOOP_KEYS})")
        lead = () if k is None else (k,)
        out = []
        for key in self.TAN_LOOP_KEYS:
            a = direction.get(key)
            if a is None:
                out.append(None)
            elif key in ("w_y", "w_u"):
                out.append(_f64(a).reshape(n, *lead, nyc if key == "w_y" else na))
            else:
                out.append(_f64(a).reshape(*lead, *shapes[key]))
        return out, (nx, ns, na)

    def run_tangent_closed_loop(self, first_order_slot: int, n_steps: int, direction=None, dx0=None, dxm1=None) -> dict:
        """The tangent of the taped closed-loop run of ``n_steps`` steps that started on ``first_order_slot``
        (``fc_run_tangent_closed_loop``) along ``direction``: a dict with any of the keys of :meth:`run_adjoint_closed_loop`'s
        gradients -- ``Ad, Bd, C, D, G, g0, S`` in the shapes :meth:`set_controllers` packs, ``x0`` (the controller's initial state),
        ``y0`` (the first measurement), ``w_y`` (n, nyc), ``w_u`` (n, n_act); absent: zero -- and ``dx0``, ``dxm1`` [N] of the two initial
        time levels.  Returns ``{"dy": (n, n_sens), "du": (n, n_act), "xi": (nx,), "dxn": (N,), "dxnm1": (N,)}``: the directional
        derivatives of the measurements, of the clamped controls (exactly 0 where a limit holds), of the controller's final state and
        of the last two time levels.  :meth:`tangent_reserve` comes first."""
        n = int(n_steps)
        arrs, (nx, ns, na) = self._tangent_loop_direction(direction, n, None)
        a = None if dx0 is None else _f64(dx0).reshape(self.N)
        b = None if dxm1 is None else _f64(dxm1).reshape(self.N)
        out = {"dy": np.zeros((n, ns)), "du": np.zeros((n, na)), "xi": np.zeros(nx), "dxn": np.empty(self.N), "dxnm1": np.empty(self.N)}
        check(self.lib.fc_run_tangent_closed_loop(self._h, int(first_order_slot), n, *(ptr(q) for q in arrs), ptr(a), ptr(b),
                                                  *(ptr(out[q]) for q in ("dy", "du", "xi", "dxn", "dxnm1"))))
        return out

    def run_tangent_closed_loop_batch(self, first_order_slot: int, n_steps: int, direction=None, dx0=None, dxm1=None, ref_col: int | None = None) -> dict:
        """k closed-loop tangents in lock step (``fc_run_tangent_closed_loop_batch``): the arrays of :meth:`run_tangent_closed_loop`
        with a leading k (``Ad`` (k, nx, nx) .., ``w_y`` (n, k, nyc), ``dx0`` (k, N)) -> ``dy`` (n, k, n_sens), ``du`` (n, k, n_act),
        ``xi`` (k, nx), ``dxn`` / ``dxnm1`` (k, N).  ``ref_col=None``: column s is the tangent of loop s; ``ref_col=c``: every column is
        a tangent of loop c along its own direction.  A column whose forward run or tangent went non-finite raises
        :class:`FcDiverged`; ``self.tangent_batch_flags`` (k,) then marks it, its entries of ``self.tangent_loop_batch_last`` are NaN
        and the other columns are valid."""
        n, k = int(n_steps), self.batch_k
        arrs, (nx, ns, na) = self._tangent_loop_direction(direction, n, k)
        a = None if dx0 is None else _f64(dx0).reshape(k, self.N)
        b = None if dxm1 is None else _f64(dxm1).reshape(k, self.N)
        out = {"dy": np.zeros((n, k, ns)), "du": np.zeros((n, k, na)), "xi": np.zeros((k, nx)), "dxn": np.empty((k, self.N)), "dxnm1": np.empty((k, self.N))}
        flags = self.tangent_batch_flags = np.zeros(max(k, 1), dtype=np.int32)
        self.tangent_loop_batch_last = out
        check(self.lib.fc_run_tangent_closed_loop_batch(self._h, int(first_order_slot), k, n, -1 if ref_col is None else int(ref_col), *(ptr(q) for q in arrs),
                                                        ptr(a), ptr(b), *(ptr(out[q]) for q in ("dy", "du", "xi", "dxn", "dxnm1")), ptr(flags)))
        return out

    # ── batched adjoint march (csrc/fc_adjoint_batch.hip.h): gradients of the k runs of set_batch in one backward sweep ──────────
    def set_adjoint_batch(self, slot: int, on: int = 1) -> None:
        """``fc_set_adjoint_batch``: 1 packs the tiled copy of ``slot``'s transposed factor values (needs :meth:`set_batch` and
        ``set_adjoint_factors(slot, 1)``) and allocates the march's ``[row][KB]`` buffers; -1 frees them."""
        check(self.lib.fc_set_adjoint_batch(self._h, int(slot), int(on)))

    def adjoint_batch_info(self, slot: int) -> dict:
        info, d = np.zeros(8, dtype=np.int64), np.zeros(2)
        check(self.lib.fc_adjoint_batch_info(self._h, int(slot), ptr(info), ptr(d)))
        return {"available": bool(info[0]), "stale": bool(info[1]), "tile_bytes": int(info[2]), "march_bytes": int(info[3]),
                "tape_bytes": int(info[4]), "repacks": int(info[5]), "KB": int(info[6]), "run_ms": float(d[0])}

    def solve_transposed_batch(self, slot: int, b) -> np.ndarray:
        """``A_slot^T X = B`` for the k columns of ``b`` (k, N) through the batched apply on the tiled transposed factors."""
        b = _f64(b).reshape(self.batch_k, self.N)
        x = np.empty_like(b)
        check(self.lib.fc_solve_transposed_batch(self._h, int(slot), self.batch_k, b, x))
        return x

    def run_adjoint_batch(self, first_order_slot: int, n_steps: int, w=None, terminal=None, state_gradients: bool = True):
        """The backward march of k lock-step forward runs of ``n_steps`` batched steps that started on ``first_order_slot``
        (``fc_run_adjoint_batch``): for ``J_s = sum_m w[m - 1, s] . y_{m,s} + terminal[s] . x_{n,s}`` returns
        ``(g [n, k, n_act], dx0 [k, N], dxm1 [k, N])`` (``None`` without ``state_gradients``).  A column that goes non-finite raises
        :class:`FcDiverged`; ``self.adjoint_batch_flags`` (k,) then marks it and ``self.adjoint_batch_last`` holds the arrays -- the
        other columns are valid."""
        n, k = int(n_steps), self.batch_k
        wq = None if w is None else _f64(w).reshape(n, k, self.n_sens)
        z = None if terminal is None else _f64(terminal).reshape(k, self.N)
        g = np.zeros((n, k, self.n_act))
        dx0, dxm1 = (np.empty((k, self.N)), np.empty((k, self.N))) if state_gradients else (None, None)
        flags = self.adjoint_batch_flags = np.zeros(max(k, 1), dtype=np.int32)
        self.adjoint_batch_last = (g, dx0, dxm1)
        check(self.lib.fc_run_adjoint_batch(self._h, int(first_order_slot), k, n, ptr(wq), ptr(z), ptr(g), ptr(dx0), ptr(dxm1), ptr(flags)))
        return g, dx0, dxm1

    def adjoint_tape_reserve_batch(self, capacity: int) -> None:
        """A state tape of ``capacity`` batched steps (``fc_adjoint_tape_reserve_batch``; 0 frees it): ``capacity + 2`` columns of
        N x KB doubles, 8 N KB bytes per step (KB: the padded width of :meth:`set_batch`, not k)."""
        check(self.lib.fc_adjoint_tape_reserve_batch(self._h, int(capacity)))

    def adjoint_tape_begin_batch(self) -> None:
        """Start taping batched steps at the present batched state (``fc_adjoint_tape_begin_batch``)."""
        check(self.lib.fc_adjoint_tape_begin_batch(self._h))

    def adjoint_tape_info_batch(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_adjoint_tape_info_batch(self._h, info))
        out = {"capacity": int(info[0]), "count": int(info[1]), "overflowed": bool(info[2]), "bytes": int(info[3]), "begun": bool(info[4]),
               "lost": int(info[5]), "KB": int(info[6])}
        if info[7] > 0:  # the checkpointed tape: its spacing, and the forward steps the last march recomputed (fc_adjoint_batch_info [7])
            binfo = np.zeros(8, dtype=np.int64)
            check(self.lib.fc_adjoint_batch_info(self._h, SLOT_BDF2, ptr(binfo), None))
            out["every"], out["replayed"] = int(info[7]), int(binfo[7])
        return out

    def adjoint_tape_reserve_sparse_batch(self, capacity: int, every: int) -> None:
        """The CHECKPOINTED batched state tape (``fc_adjoint_tape_reserve_sparse_batch``; ``every = 0`` or ``capacity = 0`` frees it):
        as :meth:`adjoint_tape_reserve_sparse` with columns of N x KB doubles and the KB control rows of every step."""
        check(self.lib.fc_adjoint_tape_reserve_sparse_batch(self._h, int(capacity), int(every)))

    def adjoint_segment_states_batch(self) -> tuple[int, np.ndarray]:
        """``(j, X)``: the segment the checkpointed batched tape's buffer holds and its ``every + 2`` columns, (every + 2, k, N) in the
        W layout (test aid, as :meth:`adjoint_segment_states`)."""
        ncol = self.adjoint_tape_info_batch()["every"] + 2
        X = np.empty((ncol, self.batch_k, self.N))
        seg = C.c_int32(0)
        check(self.lib.fc_debug_get_adjoint_segment_batch(self._h, 0, ncol, self.batch_k, X, C.byref(seg)))
        return int(seg.value), X

    def adjoint_tape_states_batch(self) -> np.ndarray:
        """The taped batched states ``x_{-1}, x_0, x_1 .. x_count`` in the W layout, (count + 2, k, N) (test aid)."""
        ncol = self.adjoint_tape_info_batch()["count"] + 2
        X = np.empty((ncol, self.batch_k, self.N))
        check(self.lib.fc_debug_get_adjoint_tape_batch(self._h, 0, ncol, self.batch_k, X))
        return X

    # ── optimal perturbations (csrc/fc_optpert.hip.h): block mass solve, resident blocks, K U = P_f Phi^T M Phi U ─────────────────
    #: the resident blocks of :meth:`optpert_reserve`
    OPTPERT_BLOCKS = {"U": 0, "G": 1, "V": 2, "R": 3, "S": 4, "Y": 5}

    def _optpert_block(self, b) -> int:
        return self.OPTPERT_BLOCKS[b] if isinstance(b, str) else int(b)

    def mass_solve_batch(self, b, rtol: float = 1e-12, max_iter: int = 500):
        """``fc_mass_solve_batch``: ``x = M_ff^-1 b_f`` for the k columns of ``b`` (k, N) by the device block CG (f: the free
        velocity rows; ``x`` is exactly zero elsewhere, what ``b`` holds there is ignored).  Returns ``(x, info [k, 2])`` with
        iterations and the final relative residual per column; ``self.mass_solve_last`` holds them when the call raises
        ``FC_ERR_NOT_CONVERGED``.  Needs :meth:`set_batch` and an assembled ``SLOT_MASS``."""
        k = self.batch_k
        b = _f64(b).reshape(k, self.N)
        x, info = np.zeros_like(b), np.zeros((max(k, 1), 2))
        self.mass_solve_last = (x, info)
        check(self.lib.fc_mass_solve_batch(self._h, k, b, x, float(rtol), int(max_iter), ptr(info)))
        return x, info

    def optpert_reserve(self, on: bool = True) -> None:
        """``fc_optpert_reserve``: the resident blocks U, G, V, R, S (scratch), Y (response) for the present batch; ``False`` frees
        everything the optimal-perturbation entry points hold."""
        check(self.lib.fc_optpert_reserve(self._h, 1 if on else 0))

    def optpert_load(self, block, X) -> None:
        """Host (k, N) -> a resident block; rows outside f are zeroed on the device."""
        check(self.lib.fc_optpert_load(self._h, self._optpert_block(block), self.batch_k, _f64(X).reshape(self.batch_k, self.N)))

    def optpert_get(self, block) -> np.ndarray:
        out = np.empty((self.batch_k, self.N))
        check(self.lib.fc_optpert_get(self._h, self._optpert_block(block), self.batch_k, out))
        return out

    def optpert_apply(self, first_order_slot: int, n_steps: int):
        """``fc_optpert_apply``: block G <- ``K U`` of block U over ``n_steps`` steps; returns ``(H [k, k] = U^T G, E [k])`` with
        ``E[c] = 1/2 x_n,c^T M x_n,c``; block Y holds ``x_n``.  Overwrites the batched state.  A non-finite column raises
        :class:`FcDiverged`; ``self.optpert_flags`` marks it and ``self.optpert_last`` holds ``(H, E)``."""
        k = self.batch_k
        H, E = np.zeros((k, k)), np.zeros(max(k, 1))
        flags = self.optpert_flags = np.zeros(max(k, 1), dtype=np.int32)
        self.optpert_last = (H, E[:k])
        check(self.lib.fc_optpert_apply(self._h, int(first_order_slot), k, int(n_steps), ptr(H), ptr(E), ptr(flags)))
        return H, E[:k]

    def optpert_mass_solve(self, dst, src, rtol: float = 1e-12, max_iter: int = 500) -> np.ndarray:
        """Block ``dst`` <- ``M_ff^-1`` block ``src`` on the device; returns info [k, 2]."""
        info = np.zeros((max(self.batch_k, 1), 2))
        check(self.lib.fc_optpert_mass_solve(self._h, self._optpert_block(dst), self._optpert_block(src), float(rtol), int(max_iter), ptr(info)))
        return info

    def optpert_gram(self, a, b, weighted: bool = False) -> np.ndarray:
        """``A^T B`` or ``A^T M B`` (k, k) of two resident blocks."""
        out = np.zeros((self.batch_k, self.batch_k))
        check(self.lib.fc_optpert_gram(self._h, self._optpert_block(a), self._optpert_block(b), 1 if weighted else 0, out))
        return out

    def optpert_combine(self, dst, src, Q, scale=None, accumulate: bool = False) -> None:
        """Block ``dst`` <- (``accumulate``: ``dst`` +) block ``src`` @ Q (k, k), columns scaled by ``scale`` (k,)."""
        k = self.batch_k
        sc = None if scale is None else _f64(scale).reshape(k)
        check(self.lib.fc_optpert_combine(self._h, self._optpert_block(dst), self._optpert_block(src), _f64(Q).reshape(k, k), ptr(sc), 1 if accumulate else 0))

    def optpert_block_raw(self, block) -> np.ndarray:
        """A resident block as it lies on the device, (N, KB) in the permuted numbering with its padding columns (test aid)."""
        KB = self.optpert_info()["KB"]
        out = np.empty((self.N, KB))
        check(self.lib.fc_debug_get_optpert_block(self._h, self._optpert_block(block), KB, out))
        return out

    def optpert_info(self) -> dict:
        info, d = np.zeros(8, dtype=np.int64), np.zeros(2)
        check(self.lib.fc_optpert_info(self._h, ptr(info), ptr(d)))
        return {"reserved": bool(info[0]), "stale": bool(info[1]), "bytes": int(info[2]), "KB": int(info[3]), "applies": int(info[4]),
                "cg_iterations": int(info[5]), "forward_steps": int(info[6]), "backward_steps": int(info[7]), "apply_ms": float(d[0]),
                "mass_solve_ms": float(d[1])}

    #: entries of :meth:`adjoint_route`
    ADJ_ROUTE_COLS = ("elem", "g_elem", "g_gather", "w", "term", "KB", "k", "g_tail", "passes", "reduced", "gx", "tape_nt")
    #: values of its ``elem`` entry: the forward element loops on the two masked levels, or the transposed-convection ones
    ADJ_ELEM = ("none", "fc_rhs_elem", "fc_rhs_elem_reg", "fc_rhs_elem_breg", "fc_adj_elem_nl", "fc_adj_elem_nl_reg", "fc_adj_elem_nl_b")
    #: ... and the ones reported only while energy weights are held (:meth:`set_adjoint_energy`), codes 7 .. 12
    ADJ_ELEM_ENERGY = ("fc_adj_elem_en", "fc_adj_elem_en_reg", "fc_adj_elem_en_b", "fc_adj_elem_nl<EN>", "fc_adj_elem_nl_reg<EN>", "fc_adj_elem_nl_b<EN>")

    # ── energy term of the marches' cost (csrc/fc_adjoint_energy.hip.h) ───────────────────────
    def set_adjoint_energy(self, e=None, batched: bool = False) -> None:
        """``fc_set_adjoint_energy``: hold the weights ``e`` of a cost term ``sum_m e[m - 1] dE_m`` (``dE_m = 1/2 x_m^T M x_m``, the
        energy every step logs) for the next marches -- ``(n,)`` for :meth:`run_adjoint` / :meth:`run_adjoint_closed_loop`, ``(n, k)``
        (or ``(n,)`` with ``batched``: every column alike) for the batched ones.  Each backward step m then adds ``e[m - 1] M x_m``
        to its right-hand side, x_m read from the state tape (which a linearised handle needs too, then).  ``None`` clears and frees
        the rows."""
        if e is None:
            check(self.lib.fc_set_adjoint_energy(self._h, 0, 0, None))
            return
        e = np.asarray(e, dtype=np.float64)
        if batched and e.ndim == 1:
            e = np.repeat(e[:, None], self.batch_k, axis=1)
        if e.ndim not in (1, 2) or e.shape[0] == 0:
            raise ValueError(f"energy weights must be (n,) or (n, k), got {e.shape}")
        e = np.ascontiguousarray(e)
        check(self.lib.fc_set_adjoint_energy(self._h, e.shape[0], 0 if e.ndim == 1 else e.shape[1], ptr(e)))

    def adjoint_energy_info(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_adjoint_energy_info(self._h, info))
        return {"n_steps": int(info[0]), "k": int(info[1]), "bytes": int(info[2]), "steps": int(info[3]), "KB": int(info[4])}

    #: values of :meth:`adjoint_route`'s ``elem`` entry reported only while the energy source is the tangent tape, codes 13 .. 16
    ADJ_ELEM_ENERGY_SOURCE = ("fc_adj_elem_en(dx)", "fc_adj_elem_en_reg(dx)", "fc_adj_elem_nl<EN, SRC>", "fc_adj_elem_nl_reg<EN, SRC>")

    def adjoint_energy_source(self) -> int:
        """The column the held weights multiply (``fc_adjoint_energy_info`` [5]): 0 the state tape's, 1 the tangent tape's."""
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_adjoint_energy_info(self._h, info))
        return int(info[5])

    def adjoint_route(self) -> np.ndarray:
        """What the last backward step of this handle launched, single or batched (``fc_get_adjoint_route``): int32 entries
        :attr:`ADJ_ROUTE_COLS`, written by the launch sites while they enqueue (test aid: a kernel, a second pass of the tail or a
        reduction that silently did not run shows here).  No launch, no synchronisation."""
        out = np.zeros(len(self.ADJ_ROUTE_COLS), dtype=np.int32)
        check(self.lib.fc_get_adjoint_route(self._h, out.size, ptr(out)))
        return out

    def adjoint_stage(self, rhs: bool = True) -> dict:
        """The buffers of the last backward step as the march holds them, in the solver's PERMUTED numbering (``self.perm``: new ->
        old; ``fc_debug_get_adjoint_stage``, test aid): ``b`` the right-hand side (``None`` without ``rhs``: a mass product overwrites
        it), ``mu`` the sum the tail formed (``x`` or ``x + dx``), ``zm`` / ``zm_prev`` the masked copy the tail wrote and the one
        before it, ``partial`` (n_act, gx) the tail's workgroup shares, ``bt`` (n_act, N) the slot's control columns, ``lift`` / ``fvec``
        (n_act, N; ``fvec`` None without force vectors) the two operands they were added from.  Call it straight after the step: a
        later solve or step of the handle reuses the buffers behind ``mu``.  After a batched
        step the vectors are (N, KB) and ``partial`` is (n_act, KB, gx)."""
        r = dict(zip(self.ADJ_ROUTE_COLS, (int(v) for v in self.adjoint_route())))
        kb, gx = r["KB"], r["g_tail"]
        shape = (self.N, kb) if kb else (self.N,)
        b = np.empty(shape) if rhs else None
        x, dx, zm, zp = (np.empty(shape) for _ in range(4))
        part = np.empty((self.n_act, kb, gx) if kb else (self.n_act, gx))
        bt, lift, fvec = (np.zeros((self.n_act, self.N)) for _ in range(3))
        has_dx, has_f = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        check(self.lib.fc_debug_get_adjoint_stage(self._h, kb, gx, ptr(b), ptr(x), ptr(dx), ptr(has_dx), ptr(zm), ptr(zp), ptr(part), ptr(bt), ptr(lift),
                                                  ptr(fvec), ptr(has_f)))
        if self.perm is None:
            self.perm = np.empty(self.N, dtype=np.int32)
            check(self.lib.fc_get_permutation(self._h, self.perm))
        return {"b": b, "mu": x + dx if has_dx[0] else x, "zm": zm, "zm_prev": zp, "partial": part, "bt": bt, "refined": bool(has_dx[0]),
                "lift": lift, "fvec": fvec if has_f[0] else None}

    # ── adjoint of a closed loop (csrc/fc_adjoint_loop.hip.h) ────────────────────────────────
    def adjoint_loop_reserve(self, capacity: int) -> None:
        """A closed-loop tape of ``capacity`` steps for the bank on the device (``fc_adjoint_loop_reserve``; 0 frees it): per step the
        controller state before its update, the measurement read and the unclamped control, ``8 (nx + n_sens + n_act)`` bytes.
        :meth:`set_controllers` comes first.  Nothing is taped before :meth:`adjoint_loop_begin`."""
        check(self.lib.fc_adjoint_loop_reserve(self._h, int(capacity)))

    def adjoint_loop_begin(self) -> None:
        """Start taping (``fc_adjoint_loop_begin``): every step of every :meth:`run_closed_loop` call from here on appends its row,
        until the bank, its state, the signals, the limits or the flow state are set anew."""
        check(self.lib.fc_adjoint_loop_begin(self._h))

    def adjoint_loop_info(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_adjoint_loop_info(self._h, info))
        return {"capacity": int(info[0]), "count": int(info[1]), "overflowed": bool(info[2]), "bytes": int(info[3]), "begun": bool(info[4]),
                "lost": int(info[5]), "bad": bool(info[6]), "row": int(info[7])}

    def run_adjoint_closed_loop(self, first_order_slot: int, n_steps: int, w=None, r=None, terminal=None, state_gradients: bool = True) -> dict:
        """The backward march over the taped closed-loop run of ``n_steps`` steps that started on ``first_order_slot``
        (``fc_run_adjoint_closed_loop``), for ``J = sum_m (w[m - 1] . y_m + r[m - 1] . u_m) + terminal . x_n``.  Returns the gradients
        with respect to the bank's matrices in the shapes :meth:`set_controllers` packs (``Ad, Bd, C, D, G, g0, S``), to the
        controller's initial state (``x0``), the first measurement (``y0``), the loop signals (``w_y`` (n, nyc), ``w_u`` (n, n_act)),
        ``ubar`` (n, n_act) = dJ/du_m of the clamped control, and ``dx0, dxm1`` (N; ``None`` without ``state_gradients``)."""
        bank = self._ctrl_bank
        if bank is None:
            raise RuntimeError("set_controllers first")
        n = int(n_steps)
        nx, nyc, nuc, ns, na = bank["nx"], bank["nyc"], bank["nuc"], self.n_sens, self.n_act
        wq = None if w is None else _f64(w).reshape(n, ns)
        rq = None if r is None else _f64(r).reshape(n, na)
        z = None if terminal is None else _f64(terminal).reshape(self.N)
        out = {"Ad": np.zeros((nx, nx)), "Bd": np.zeros((nx, nyc)), "C": np.zeros((nuc, nx)), "D": np.zeros((nuc, nyc)), "G": np.zeros((nyc, ns)),
               "g0": np.zeros(nyc), "S": np.zeros((na, nuc)), "x0": np.zeros(nx), "y0": np.zeros(ns), "w_y": np.zeros((n, nyc)),
               "w_u": np.zeros((n, na)), "ubar": np.zeros((n, na))}
        out["dx0"], out["dxm1"] = (np.empty(self.N), np.empty(self.N)) if state_gradients else (None, None)
        order = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "ubar", "dx0", "dxm1")
        check(self.lib.fc_run_adjoint_closed_loop(self._h, int(first_order_slot), n, ptr(wq), ptr(rq), ptr(z), *(ptr(out[k]) for k in order)))
        return out

    # ── adjoint of k lock-step closed loops (csrc/fc_adjoint_loop_batch.hip.h) ───────────────
    def adjoint_loop_reserve_batch(self, capacity: int) -> None:
        """A loop tape of ``capacity`` steps for the bank of ``batch_k`` controllers on the device (``fc_adjoint_loop_reserve_batch``;
        0 frees it): ``8 k (nx + n_sens + n_act)`` bytes per step, and an untransposed copy of the bank.  :meth:`set_batch` and
        :meth:`set_controllers` with ``batch_k`` controllers come first.  Nothing is taped before :meth:`adjoint_loop_begin_batch`."""
        check(self.lib.fc_adjoint_loop_reserve_batch(self._h, int(capacity)))

    def adjoint_loop_begin_batch(self) -> None:
        """Start taping (``fc_adjoint_loop_begin_batch``): every step of every :meth:`run_closed_loop_batch` call from here on appends
        one row per simulation -- and the new state to a begun batched state tape -- until the bank, its state, the signals, the
        limits or the batched state are set anew or a batched step is taken outside the loop."""
        check(self.lib.fc_adjoint_loop_begin_batch(self._h))

    def adjoint_loop_info_batch(self) -> dict:
        info = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_adjoint_loop_info_batch(self._h, info))
        return {"capacity": int(info[0]), "count": int(info[1]), "overflowed": bool(info[2]), "bytes": int(info[3]), "begun": bool(info[4]),
                "lost": int(info[5]), "bad": int(info[6]), "row": int(info[7])}

    def run_adjoint_closed_loop_batch(self, first_order_slot: int, n_steps: int, w=None, r=None, terminal=None, state_gradients: bool = True) -> dict:
        """The backward march over the taped run of ``n_steps`` batched closed-loop steps that started on ``first_order_slot``
        (``fc_run_adjoint_closed_loop_batch``), for ``J_s = sum_m (w[m - 1, s] . y_{m,s} + r[m - 1, s] . u_{m,s}) + terminal[s] . x_{n,s}``:
        the dict of :meth:`run_adjoint_closed_loop` with a leading k on every array -- ``Ad`` (k, nx, nx) .. ``S`` (k, n_act, nuc), ``x0``
        (k, nx), ``y0`` (k, n_sens), ``w_y`` (n, k, nyc), ``w_u`` / ``ubar`` (n, k, n_act), ``dx0`` / ``dxm1`` (k, N; ``None`` without
        ``state_gradients``).  A column whose forward run or adjoint went non-finite raises :class:`FcDiverged`;
        ``self.adjoint_batch_flags`` (k,) then marks it, its entries of ``self.adjoint_loop_batch_last`` are NaN and the other columns
        are valid."""
        bank = self._ctrl_bank
        if bank is None:
            raise RuntimeError("set_controllers first")
        n, k = int(n_steps), self.batch_k
        nx, nyc, nuc, ns, na = bank["nx"], bank["nyc"], bank["nuc"], self.n_sens, self.n_act
        wq = None if w is None else _f64(w).reshape(n, k, ns)
        rq = None if r is None else _f64(r).reshape(n, k, na)
        z = None if terminal is None else _f64(terminal).reshape(k, self.N)
        out = {"Ad": np.zeros((k, nx, nx)), "Bd": np.zeros((k, nx, nyc)), "C": np.zeros((k, nuc, nx)), "D": np.zeros((k, nuc, nyc)),
               "G": np.zeros((k, nyc, ns)), "g0": np.zeros((k, nyc)), "S": np.zeros((k, na, nuc)), "x0": np.zeros((k, nx)), "y0": np.zeros((k, ns)),
               "w_y": np.zeros((n, k, nyc)), "w_u": np.zeros((n, k, na)), "ubar": np.zeros((n, k, na))}
        out["dx0"], out["dxm1"] = (np.empty((k, self.N)), np.empty((k, self.N))) if state_gradients else (None, None)
        order = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "ubar", "dx0", "dxm1")
        flags = self.adjoint_batch_flags = np.zeros(max(k, 1), dtype=np.int32)
        self.adjoint_loop_batch_last = out
        check(self.lib.fc_run_adjoint_closed_loop_batch(self._h, int(first_order_slot), k, n, ptr(wq), ptr(rq), ptr(z), *(ptr(out[q]) for q in order),
                                                        ptr(flags)))
        return out

    # ── closed loop on the device (controller bank, csrc/fc_ctrl.hip.h) ──────────────────────
    def set_controllers(self, controllers, dt: float, feedback=None) -> dict | None:
        """Put the discrete forms (ZOH at ``dt``) of ``controllers`` — one per simulation: a single one for :meth:`run_closed_loop`,
        ``batch_k`` for :meth:`run_closed_loop_batch` — on the device with their current states (``fc_set_controllers``).
        ``feedback``: ``None`` (``yc = -y_meas[0]``) or ``(G, g0)``.  ``None`` / an empty list frees the bank.  Returns the packed bank
        (:func:`flowcontrol_amd.controller.pack_controllers`)."""
        from .controller import pack_controllers

        if not controllers:
            check(self.lib.fc_set_controllers(self._h, 0, 0, 1, 1, None, None, None, None, None, None, None, None))
            self._ctrl_bank = None
            return None
        bank = pack_controllers(controllers, dt, self.n_sens, self.n_act, feedback)
        check(self.lib.fc_set_controllers(self._h, bank["k"], bank["nx"], bank["nyc"], bank["nuc"], ptr(_f64(bank["Ad"])), ptr(_f64(bank["Bd"])),
                                          ptr(_f64(bank["C"])), ptr(_f64(bank["D"])), ptr(_f64(bank["x0"])), ptr(_f64(bank["G"])),
                                          ptr(_f64(bank["g0"])), ptr(_f64(bank["S"]))))
        self._ctrl_bank = bank
        return bank

    def controller_state(self, x=None) -> np.ndarray:
        """States (k, nx) of the bank's controllers, zero-padded to the bank's ``nx``; with ``x``: set them first
        (``fc_set_controller_state``: a new run)."""
        bank = self._ctrl_bank
        if bank is None:
            raise RuntimeError("set_controllers first")
        k, nx = bank["k"], bank["nx"]
        if x is not None:
            xs = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(k, nx))
            check(self.lib.fc_set_controller_state(self._h, k, ptr(xs)))
        out = np.zeros((k, nx))
        check(self.lib.fc_get_controller_state(self._h, k, ptr(out)))
        return out

    def ctrl_apply(self, y) -> np.ndarray:
        """Advance the bank once from the measurements ``y`` (k, n_sens); returns u (k, n_act) (``fc_ctrl_apply``)."""
        k = self._ctrl_bank["k"]
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(k, self.n_sens))
        u = np.empty((k, self.n_act))
        check(self.lib.fc_ctrl_apply(self._h, k, y, u))
        return u

    def set_loop_signals(self, w_y=None, w_u=None) -> None:
        """Signals added to the loop of the bank (``fc_set_loop_signals``): ``w_y`` (n, k, nyc) at the controller input, ``w_u``
        (n, k, n_act) at the plant input (k = 1: the middle axis may be left out); either may be ``None``, both ``None`` frees them.
        The rows stay on the device; the handle's cursor (:meth:`loop_cursor`) starts at row 0 and every closed-loop call reads on
        from it."""
        bank = self._ctrl_bank
        if bank is None:
            raise RuntimeError("set_controllers first")
        k = bank["k"]
        n = None
        arrs = []
        for w, width, name in ((w_y, bank["nyc"], "w_y"), (w_u, self.n_act, "w_u")):
            if w is None:
                arrs.append(None)
                continue
            w = np.asarray(w, dtype=np.float64)
            if w.ndim == 2 and k == 1:
                w = w[:, None, :]
            if w.ndim != 3 or w.shape[1:] != (k, width):
                raise ValueError(f"{name} must have shape (n, {k}, {width}), got {w.shape}")
            if n is not None and w.shape[0] != n:
                raise ValueError("w_y and w_u must have the same number of rows")
            n = w.shape[0]
            arrs.append(np.ascontiguousarray(w))
        check(self.lib.fc_set_loop_signals(self._h, k, int(n or 0), ptr(arrs[0]), ptr(arrs[1])))

    def set_control_limits(self, lo=None, hi=None) -> None:
        """Actuator limits of the bank (``fc_set_control_limits``): ``u = min(max(v, lo), hi)``; scalars, per actuator (n_act,) or per
        simulation and actuator (k, n_act); ±inf leaves that side free.  Both ``None``: no limits."""
        bank = self._ctrl_bank
        if bank is None:
            raise RuntimeError("set_controllers first")
        k = bank["k"]
        if lo is None and hi is None:
            check(self.lib.fc_set_control_limits(self._h, k, None, None))
            return
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), (k, self.n_act)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), (k, self.n_act)))
        check(self.lib.fc_set_control_limits(self._h, k, ptr(lo), ptr(hi)))

    def loop_cursor(self) -> int:
        """The row of the loop signals that the next closed-loop step reads (``fc_get_loop_cursor``)."""
        row = C.c_int64(0)
        check(self.lib.fc_get_loop_cursor(self._h, C.byref(row)))
        return int(row.value)

    def run_monitor(self) -> dict:
        """What the residual monitor saw over the last closed-loop run (``fc_get_run_monitor``)."""
        r, a, b = C.c_double(), C.c_int32(), C.c_int32()
        check(self.lib.fc_get_run_monitor(self._h, C.byref(r), C.byref(a), C.byref(b)))
        return {"max_residual": r.value, "residual_step": a.value, "first_bad_step": b.value}

    def run_closed_loop(self, first_order_slot: int, n_steps: int, y0, compute_energy: bool = True):
        """``n_steps`` closed-loop steps with the bank's controller, no host synchronisation in between (``fc_run_closed_loop``):
        ``(y [n, n_sens], u [n, n_act], dE [n])``.  On :class:`FcDiverged` the rows up to the failed step are in
        ``self._closed_loop_rows`` and :meth:`run_monitor` names the step."""
        y0 = np.ascontiguousarray(np.asarray(y0, dtype=np.float64).reshape(self.n_sens))
        y, u, dE = np.empty((n_steps, self.n_sens)), np.empty((n_steps, self.n_act)), np.empty(n_steps)
        self._closed_loop_rows = (y, u, dE)
        check(self.lib.fc_run_closed_loop(self._h, first_order_slot, n_steps, y0, ptr(y), ptr(u), ptr(dE), int(compute_energy)))
        return y, u, dE

    def run_closed_loop_batch(self, first_order_slot: int, n_steps: int, y0, compute_energy: bool = True):
        """The same for the batch: ``(y [n, k, n_sens], u [n, k, n_act], dE [n, k], first_bad_step [k], info [k, 4])``; a non-finite run
        does not raise here — ``first_bad_step`` names its step (-1: finite to the end), the other runs are unaffected."""
        k = self.batch_k
        y0 = np.ascontiguousarray(np.asarray(y0, dtype=np.float64).reshape(k, self.n_sens))
        y, u, dE = np.empty((n_steps, k, self.n_sens)), np.empty((n_steps, k, self.n_act)), np.empty((n_steps, k))
        bad, info = np.full(k, -1, dtype=np.int32), np.empty((k, 4))
        code = self.lib.fc_run_closed_loop_batch(self._h, first_order_slot, k, n_steps, y0, ptr(y), ptr(u), ptr(dE), int(compute_energy), ptr(bad),
                                                 ptr(info))
        if code != _lib.FC_ERR_DIVERGED:
            check(code)
        return y, u, dE, bad, info

    # ── shared-operator batched stepping (k lock-step simulations on this handle) ────────────
    def set_batch(self, k: int) -> None:
        """Allocate (k > 0) or free (k = 0) the state of k lock-step simulations that share this handle's operators and
        factors (``fc_set_batch``): IC sweeps / controller sweeps of the reference run k FlowSolver instances instead."""
        check(self.lib.fc_set_batch(self._h, int(k)))
        self.batch_k = int(k)
        self._batch_bufs = None

    def set_state_batch(self, u_n, u_nn, p_n=None) -> None:
        k = self.batch_k
        u_n, u_nn = _f64(u_n).reshape(k, 2 * self.nn), _f64(u_nn).reshape(k, 2 * self.nn)
        p = None if p_n is None else _f64(p_n).reshape(k, self.th.nv)
        check(self.lib.fc_set_state_batch(self._h, k, u_n, u_nn, ptr(p)))

    def get_state_batch(self):
        k = self.batch_k
        u_n, u_nn, p_n = np.empty((k, 2 * self.nn)), np.empty((k, 2 * self.nn)), np.empty((k, self.th.nv))
        check(self.lib.fc_get_state_batch(self._h, k, ptr(u_n), ptr(u_nn), ptr(p_n)))
        return u_n, u_nn, p_n

    def get_solution_batch(self) -> np.ndarray:
        up = np.empty((self.batch_k, self.N))
        check(self.lib.fc_get_solution_batch(self._h, self.batch_k, up))
        return up

    def _batch_buffers(self):
        b = self._batch_bufs
        if b is None:
            k = self.batch_k
            arrs = (np.zeros((k, max(self.n_act, 1))), np.zeros((k, max(self.n_act, 1))), np.empty((k, max(self.n_sens, 1))), np.empty(k),
                    np.empty((k, 4)))
            b = self._batch_bufs = arrs + (tuple(ptr(a) for a in arrs),)
        return b

    def step_batch_begin(self, order_slot: int, u_ctrl, compute_energy: bool = True, u_force=None) -> None:
        u, uf, y, dE, info, (pu, puf, py, pdE, pinfo) = self._batch_buffers()
        if self.n_act:
            u[:, : self.n_act] = np.asarray(u_ctrl, dtype=np.float64).reshape(self.batch_k, self.n_act)
            if u_force is not None:
                uf[:, : self.n_act] = np.asarray(u_force, dtype=np.float64).reshape(self.batch_k, self.n_act)
        code = self.lib.fc_step_batch_begin(self._h, order_slot, self.batch_k, pu if self.n_act else None,
                                            puf if (self.n_act and u_force is not None) else None, 1 if compute_energy else 0)
        if code:
            check(code)

    def step_batch_end(self):
        """(y [k, n_sens], dE [k], info [k, 4]) of the step in flight; raises :class:`FcDiverged` if any simulation
        produced a non-finite velocity (``info[:, 3]`` of ``self._batch_bufs`` marks which)."""
        u, uf, y, dE, info, (pu, puf, py, pdE, pinfo) = self._batch_bufs
        code = self.lib.fc_step_batch_end(self._h, self.batch_k, py, pdE, pinfo)
        if code:
            check(code)
        return y[:, : self.n_sens].copy(), dE.copy(), info

    def step_batch_end_early(self):
        """(y [k, n_sens], flags [k]) as soon as the batched solve is done; energy and solve info follow (:meth:`step_batch_collect`).
        Raises :class:`FcDiverged` if any simulation produced a non-finite velocity (``self._batch_flags`` marks which)."""
        u, uf, y, dE, info, (pu, puf, py, pdE, pinfo) = self._batch_bufs
        if getattr(self, "_batch_flags", None) is None or self._batch_flags.size != self.batch_k:
            self._batch_flags = np.zeros(self.batch_k, dtype=np.int32)
        code = self.lib.fc_step_batch_end_early(self._h, self.batch_k, py, ptr(self._batch_flags))
        if code:
            check(code)
        return y[:, : self.n_sens].copy(), self._batch_flags

    def step_batch_collect(self):
        """(dE [k], info [k, 4]) of the last batched step that ended early; blocks until they exist."""
        u, uf, y, dE, info, (pu, puf, py, pdE, pinfo) = self._batch_bufs
        check(self.lib.fc_step_batch_collect(self._h, self.batch_k, pdE, pinfo))
        return dE.copy(), info

    def step_batch(self, order_slot: int, u_ctrl, compute_energy: bool = True, u_force=None):
        """One blocking batched step: (y, dE, info), all waited for."""
        self.step_batch_begin(order_slot, u_ctrl, compute_energy, u_force)
        return self.step_batch_end()

    def reset_sim_batch(self, s: int) -> None:
        """``fc_reset_sim_batch``: take simulation ``s`` (e.g. one that diverged) out of the batch's dynamics — zero state, flag cleared."""
        check(self.lib.fc_reset_sim_batch(self._h, int(s)))

    def batch_info(self) -> dict:
        a = np.zeros(8)
        check(self.lib.fc_get_batch_info(self._h, a))
        return {"k": int(a[0]), "KB": int(a[1]), "scratch_rows": int(a[2]), "block_launches": int(a[3]), "fold_launches": int(a[4]),
                "factor_bytes": a[5], "vector_bytes": a[6], "tasks": int(a[7])}

    #: columns of :meth:`batch_launches`
    BATCH_LAUNCH_COLS = ("kind", "count", "cg", "min", "max", "split", "parts", "nontemporal")

    def batch_launches(self, slot: int = SLOT_BDF2) -> np.ndarray:
        """What the batched factor apply launches for ``slot`` at the current batch width, in launch order (``fc_get_batch_launches``):
        one int32 row per launch, columns :attr:`BATCH_LAUNCH_COLS` — block launches ``(0, tasks, column-group waves, fewest / most
        32-column chunks of a task, split tiles present, most parts of a tile, nontemporal loads)``, fold launches ``(1, rows, 0, fewest /
        most source rows of a row, 0, 0, 0)``: which branches of the block and fold kernels ran."""
        info = self.batch_info()
        out = np.zeros((info["block_launches"] + info["fold_launches"], len(self.BATCH_LAUNCH_COLS)), dtype=np.int32)
        check(self.lib.fc_get_batch_launches(self._h, slot, out.size, out.reshape(-1)))
        return out

    def bench_batch_apply(self, slot: int, reps: int = 200) -> float:
        ms = C.c_double()
        check(self.lib.fc_bench_batch_apply(self._h, slot, reps, C.byref(ms)))
        return ms.value

    def solve_batch(self, slot: int, b) -> np.ndarray:
        b = _f64(b).reshape(self.batch_k, self.N)
        x = np.empty_like(b)
        check(self.lib.fc_solve_batch(self._h, slot, self.batch_k, b, x))
        return x

    # ── parity hooks ─────────────────────────────────────────────────────────
    def assemble_rhs(self, order_slot: int, u_ctrl) -> np.ndarray:
        u = _f64(np.atleast_1d(u_ctrl)) if self.n_act else None
        b = np.empty(self.N)
        check(self.lib.fc_assemble_rhs(self._h, order_slot, ptr(u), b))
        return b

    def solve(self, slot: int, b):
        x = np.empty(self.N)
        info = np.empty(4)
        code = self.lib.fc_solve(self._h, slot, _f64(b), x, ptr(info))
        self._raise_exchange_error()
        check(code)
        return x, info

    def energy(self, u) -> float:
        E = C.c_double()
        check(self.lib.fc_energy(self._h, _f64(u), C.byref(E)))
        return E.value

    def measure(self, up) -> np.ndarray:
        y = np.empty(max(self.n_sens, 1))
        check(self.lib.fc_measure(self._h, _f64(up), ptr(y)))
        return y[: self.n_sens]

    # ── measurement ──────────────────────────────────────────────────────────
    def bench_sweeps(self, slot: int, reps: int = 200):
        ms, nl = C.c_double(), C.c_int32()
        check(self.lib.fc_bench_sweeps(self._h, slot, reps, C.byref(ms), C.byref(nl)))
        return ms.value, nl.value

    #: columns of :meth:`sweep_launches`
    SWEEP_LAUNCH_COLS = ("kernel", "direction", "p1", "p2", "workgroups", "nontemporal", "bits", "rows")
    #: values of the ``kernel`` column
    SWEEP_KERNELS = ("fc_nd_sweep", "fc_nd_down_block", "fc_nd_flat_block", "fc_nd_fold1", "fc_diag_stage")

    def sweep_launches(self, slot: int = SLOT_BDF2) -> np.ndarray:
        """What one whole single-vector factor apply of ``slot`` launches, in launch order (``fc_get_sweep_launches``): one int32 row per
        launch, columns :attr:`SWEEP_LAUNCH_COLS` — kernel (index into :attr:`SWEEP_KERNELS`), direction (0 up, 1 down), the kernel's
        template parameters (LANES, SUB / LPR, RPS / loads per thread), workgroups, nontemporal loads, storage bits, rows written.  It is
        the record the launchers switch on: which template instances ran."""
        n = self.lib.fc_get_sweep_launches(self._h, slot, 0, None)  # (n = 0: the number of launches, or an error code < 0)
        if n < 0:
            check(n)
        out = np.zeros((n, len(self.SWEEP_LAUNCH_COLS)), dtype=np.int32)
        if n:
            check(self.lib.fc_get_sweep_launches(self._h, slot, out.size, ptr(out)))
        return out

    #: entries of :meth:`step_route`
    STEP_ROUTE_COLS = ("elem", "speculated", "solver", "tail", "monitored", "g_rows", "g_check", "g_cells", "reps")
    STEP_ELEM = ("reused", "fc_rhs_elem", "fc_rhs_elem_reg")
    STEP_SOLVERS = ("apply", "refine", "bicgstab", "gmres")
    STEP_TAILS = ("fc_tail+fc_final", "fc_tail<fused final>", "fc_finish+fc_final", "fc_early+side stream")

    def step_route(self) -> np.ndarray:
        """What the last time step of this handle launched (``fc_get_step_route``): int32 entries :attr:`STEP_ROUTE_COLS` -- element
        kernel (index into :attr:`STEP_ELEM`), slot speculated for the next step or -1, solver (:attr:`STEP_SOLVERS`), tail
        (:attr:`STEP_TAILS`), whether the residual was monitored, row / check / cell workgroups of the tail and its groups per
        workgroup.  Written by the launch sites themselves: which kernels ran."""
        out = np.zeros(len(self.STEP_ROUTE_COLS), dtype=np.int32)
        check(self.lib.fc_get_step_route(self._h, out.size, ptr(out)))
        return out

    #: entries of :meth:`batch_step_route`
    BATCH_ROUTE_COLS = ("lead", "elem", "spec", "spec_gather", "overlapped", "late_gate", "monitored", "n_row_blocks", "n_cell_blocks", "tb_cols", "KB",
                        "n_ctrl_rows", "graph")
    BATCH_ELEM = ("none", "fc_rhs_elem_b", "fc_rhs_elem_breg", "fc_rhs_elem_breg<FORCE>")

    def batch_step_route(self) -> np.ndarray:
        """What the last batched step of this handle launched (``fc_get_batch_step_route``): int32 entries :attr:`BATCH_ROUTE_COLS` --
        how the step began (2 element loop, 1 full gather, 0 control rows only), the element kernel it launched (index into
        :attr:`BATCH_ELEM`), slot + 1 speculated for the next step and whether its gather ran ahead, overlapped or one stream, the late
        gate, whether the residual was monitored, row blocks / cell workgroups / column width of the tail, the padded width, the slot's
        control rows, graph replay.  Written where the dispatch decides: which kernels ran."""
        out = np.zeros(len(self.BATCH_ROUTE_COLS), dtype=np.int32)
        check(self.lib.fc_get_batch_step_route(self._h, out.size, ptr(out)))
        return out

    def capture_batch_rhs(self, on: bool = True) -> None:
        """``fc_debug_capture_batch_rhs`` (test aid): every batched step from here on keeps a copy of the right-hand side its solve consumed."""
        check(self.lib.fc_debug_capture_batch_rhs(self._h, int(bool(on))))

    def batch_rhs(self) -> np.ndarray:
        """The right-hand side the last batched step's solve consumed, (k, N) in the W layout (``fc_debug_get_batch_rhs``)."""
        out = np.empty((self.batch_k, self.N))
        check(self.lib.fc_debug_get_batch_rhs(self._h, self.batch_k, ptr(out)))
        return out

    PHASES = ("rhs", "up_sweeps", "exchange1", "root", "exchange2", "down_sweeps", "tail", "exchange3", "publish")

    def set_phase_timing(self, on: bool) -> None:
        """HIP-event marks at the phase boundaries of every ``fc_step`` from now on (an instrumented replay, see fc_hip_internal.h)."""
        check(self.lib.fc_set_phase_timing(self._h, int(bool(on))))

    def get_phase_timing(self) -> dict:
        """Mean microseconds per step of every phase since :meth:`set_phase_timing`, keyed by :attr:`PHASES`, plus ``steps``."""
        us, n = np.zeros(len(self.PHASES)), C.c_int64()
        check(self.lib.fc_get_phase_timing(self._h, us, C.byref(n)))
        d = {k: float(v) / max(n.value, 1) for k, v in zip(self.PHASES, us)}
        d["steps"] = int(n.value)
        return d

    def set_timing(self, on: bool) -> None:
        check(self.lib.fc_set_timing(self._h, int(bool(on))))

    def get_timing(self) -> dict:
        a, b = C.c_double(), C.c_double()
        na, nb = C.c_int64(), C.c_int64()
        check(self.lib.fc_get_timing(self._h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return {"sweep_ms": a.value, "sweep_launches": na.value, "spmv_ms": b.value, "spmv_launches": nb.value}

    def algorithmic_bytes(self, slot: int):
        a, b = C.c_double(), C.c_double()
        check(self.lib.fc_algorithmic_bytes(self._h, slot, C.byref(a), C.byref(b)))
        return a.value, b.value


__all__ = ["DeviceSolver", "SLOT_BDF1", "SLOT_BDF2", "SLOT_MASS", "SLOT_SCRATCH"]
