"""The sharded route of expected hypervolume improvement on CPU: PointSelector's own reduction - idx_offset = the shard's first
candidate, the arg-max records folded over the ranks, the dense array gathered in rank order - with the device call stubbed and a
real 2-process gloo group (the GPU path uses the same code over RCCL).  Both ranks must return the single-process answer: the
LOWEST index of a maximum attained in both shards, index 0 when every value is -inf, the NaN counts added."""
import os
import socket
from types import SimpleNamespace

import numpy as np

FD = [5, 7]
M = 35
Y1, Y2 = [1.0, 2.0, 3.0], [6.0, 5.0, 5.5]                    # the observed pairs: (3, 5.5) is dominated by (2, 5)
FRONT, REF = [[1.0, 6.0], [2.0, 5.0]], (3.0 + 0.1 * 2.0, 6.0 + 0.1 * 1.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scores(case):
    """log EHVI [M] over ALL candidates of a case; a rank's stub returns its slice."""
    val = -np.arange(M, dtype=np.float64) - 1700.0         # far below where the plain sum is 0
    if case == "tie":
        val[[9, 30]] = -1.5                                # the maximum, once in each shard (18 | 17 candidates): 9 wins
        val[[0, 34]] = -np.inf
    elif case == "all_minus_inf":
        val[:] = -np.inf
    elif case == "nan":
        val[9], val[20], val[21] = -1.5, np.nan, np.nan    # both NaN in the second shard
    return val


class _StubGP:
    """Stands in for DeviceGP: the local record the kernel would return for this shard, on CPU tensors."""

    def __init__(self, case):
        import torch

        self.torch, self.case, self.calls = torch, case, []

    def ehvi_on_posterior(self, mu1, sigma1, mu2, sigma2, front, ref, idx_offset, dense):
        n = int(mu1.shape[0])
        self.calls.append((idx_offset, n, int(mu2.shape[0]), np.asarray(front).tolist(), tuple(ref), dense))
        val = _scores(self.case)[idx_offset: idx_offset + n]
        ok = ~np.isnan(val)
        best = val[ok].max()
        idx = idx_offset + int(np.flatnonzero(ok & (val == best))[0])
        return SimpleNamespace(best_val=float(best), best_idx=idx, nan_count=int((~ok).sum()), value=self.torch.from_numpy(val.copy()))


def _selector(case, lo, hi, y):
    import torch

    from bayesian_optimisation_amd import PointSelector

    ps = PointSelector()
    ps.feature_domain = FD
    ps.predicted_pts = np.stack(np.meshgrid(np.linspace(0, 1, 5), np.linspace(0, 1, 7), indexing="ij"), -1).reshape(-1, 2)
    ps.measured_pts, ps.measured_vals = [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]], y
    ps._cached, ps._lo_hi = {}, (lo, hi)
    ps._gp = _StubGP(case)
    ps._mu_dev, ps._sigma_dev = torch.zeros(hi - lo, dtype=torch.float64), torch.ones(hi - lo, dtype=torch.float64)
    return ps


def _run_cases(rank, world):
    from bayesian_optimisation_amd import distributed as D

    lo, hi = D.shard_bounds(M, world, rank)
    out = {}
    for case in ("tie", "all_minus_inf", "nan"):
        obj, other = _selector(case, lo, hi, Y1), _selector(case, lo, hi, Y2)
        try:
            idx = obj.expected_hypervolume_improvement(other).tolist()
        except IndexError as exc:
            idx = "IndexError: " + str(exc)[:12]
        out[case] = (idx, obj.acq_func_eval.tobytes(), obj.pareto_front.tolist(), obj.reference_point, obj.hypervolume,
                     obj._gp.calls, other._gp.calls)
    return out


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run_cases(rank, world)))
    finally:
        dist.destroy_process_group()


def _check(out, lo, hi):
    for case, want in (("tie", [1, 2]), ("all_minus_inf", [0, 0]), ("nan", None)):
        idx, acq, front, ref, hv, calls, other_calls = out[case]
        assert idx == want if want is not None else idx.startswith("IndexError"), (case, idx)
        assert acq == _scores(case).reshape(FD).tobytes()                                # gathered in rank order, bytes unchanged
        assert front == FRONT and ref == REF                                             # the observed front below the nadir point
        assert abs(hv - ((2.0 - 1.0) * (REF[1] - 6.0) + (REF[0] - 2.0) * (REF[1] - 5.0))) <= 1e-14
        assert calls == [(lo, hi - lo, hi - lo, FRONT, REF, True)] and other_calls == []  # one call, idx_offset = the shard's start


def test_two_ranks_return_the_single_process_answer():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(res) == [0, 1]
    _check(res[0], 0, 18)
    _check(res[1], 18, 35)


def test_one_process_is_the_same_route():
    _check(_run_cases(0, 1), 0, M)
