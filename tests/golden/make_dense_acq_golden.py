"""Records tests/golden/dense_acq_bits.json: the bits the four acquisitions on the dense posterior give on an MI355X, through the
public C entries (gpbo_acq_argmax_f64, gpbo_mes_acq_f64, gpbo_constrained_acq_f64, gpbo_ehvi_acq_f64), for
tests/test_gpu_dense_acq.py, which imports the inputs, the cases and the runner from here and asserts equality.

    python tests/golden/make_dense_acq_golden.py [OUT.json]        (needs the GPU and the built library)

The fixture was recorded at the commit BEFORE the four kernels became instances of dense_acq_kernel (csrc/dense_acq.h): it is
what that refactor, and every later change of the frame or of a score functor, has to reproduce.  Record it again only where a
change of the arithmetic is the purpose of a commit, and from the commit before it wherever the purpose is anything else.

Inputs are exact integer arithmetic: a multiplicative hash of the index mod 2^32, scaled by powers of two - no RNG and no libm, so
they are the same on every machine and are not stored.  Per case the fixture holds the SHA-256 of each dense output's bytes,
best_val as a hex bit pattern, best_idx and nan_count."""
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "dense_acq_bits.json")
# one lane; a masked tail; an exact workgroup; one candidate into a second workgroup; one candidate into the second grid-stride
# trip of workgroup 0 (1024 workgroups x 256 + 1)
SIZES = [1, 255, 256, 257, 262145]
OFFSET = (3 << 32) + 17
NAN_AT = (0, 63, 64, -1)          # both sides of a wave boundary and the last candidate
ZERO_SIGMA_AT = (5, 100, 200)
TIE_AT = (37, -3)                  # the best value twice: a low and a high index
SENTINEL = 12345.0                 # what a dense output holds before the call: an element the kernel skips stays visible
CONS_C = 8


def _hash(i, salt):
    """32 well-mixed bits of (i, salt) in [0, 1): exact in fp64."""
    m = np.uint64(0xFFFFFFFF)
    x = (i.astype(np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(2246822519)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) * 2.0 ** -32


def _mean(n, salt):      # in [-4, 4)
    return (_hash(np.arange(n), salt) - 0.5) * 8.0


def _sigma(n, salt):     # in [2^-6, 2 + 2^-6)
    return _hash(np.arange(n), salt) * 2.0 + 2.0 ** -6


def inputs(M, plant=True):
    """mu, sigma, mu2, sigma2 [M]; cons_mu, cons_sigma [CONS_C x ldc] flat, ldc = M + 5.  plant: the NaNs, zero sigmas and the tie
    at every listed index the size has room for (M == 1 is then one NaN candidate: the empty record)."""
    ldc = M + 5
    a = {"mu": _mean(M, 1), "sigma": _sigma(M, 2), "mu2": _mean(M, 3), "sigma2": _sigma(M, 4),
         "cons_mu": _mean(CONS_C * ldc, 5).reshape(CONS_C, ldc), "cons_sigma": _sigma(CONS_C * ldc, 6).reshape(CONS_C, ldc)}
    if plant:
        for j in ZERO_SIGMA_AT:
            if j < M:
                a["sigma"][j], a["sigma2"][j + 1 if j + 1 < M else j] = 0.0, 0.0
                a["cons_sigma"][j % CONS_C, j], a["cons_sigma"][(j + 3) % CONS_C, j + 2 if j + 2 < M else j] = 0.0, 0.0
        if M > 80:
            for j in TIE_AT:
                a["mu"][j], a["sigma"][j], a["mu2"][j], a["sigma2"][j] = -100.0, 1.0, -100.0, 1.0
                a["cons_mu"][:, j % M], a["cons_sigma"][:, j % M] = -100.0, 1.0
        for k, j in enumerate(NAN_AT):
            if j < M:
                a[("mu", "sigma")[k % 2]][j] = np.nan
                a[("cons_mu", "cons_sigma")[k % 2]][(0, 7, 3, 0)[k], j % M] = np.nan
        if M > 65:   # the second objective: one NaN beside one of the first (counted once), one of its own
            a["mu2"][63], a["sigma2"][65] = np.nan, np.nan
    a["cons_mu"], a["cons_sigma"], a["ldc"] = a["cons_mu"].reshape(-1), a["cons_sigma"].reshape(-1), ldc
    return a


def front(P):
    """(front [P x 2] strictly ascending / descending, ref1, ref2), every value a multiple of 2^-6."""
    i = np.arange(P, dtype=np.float64)
    return np.ascontiguousarray(np.stack([-2.0 + i / 64.0, 1.0 - i / 64.0], axis=1)), 0.5, 1.5


def cases():
    """(entry, parameters) of every call, in fixture order; each runs with and without its dense outputs."""
    out = [("acq", {"kind": k}) for k in ("lcb", "ei")]
    out += [("mes", {"S": S}) for S in (1, 64)]
    # (base none with no constraint reads no input array at all, and the entry refuses it)
    out += [("cons", {"base": b, "C": C}) for b in ("none", "ei", "pi") for C in (0, CONS_C) if (b, C) != ("none", 0)]
    out += [("ehvi", {"P": P}) for P in (0, 128)]
    return out


def case_id(entry, par, M, plant, dense):
    tag = "-".join(f"{k}={v}" for k, v in sorted(par.items()))
    return f"{entry}:{tag}:M={M}:{'planted' if plant else 'clean'}:{'dense' if dense else 'record'}"


def size_variants():
    """(M, plant): every size planted, and M = 1 also clean (planted it is a single NaN candidate)."""
    return [(M, True) for M in SIZES] + [(1, False)]


class Runner:
    """The device copies of one (M, plant) input set and the calls on them."""

    def __init__(self, M, plant, device="cuda:0"):
        import torch

        from bayesian_optimisation_amd import _lib

        self.torch, self.L, self.lib, self.M, self.device = torch, _lib, _lib.load(), M, device
        host = inputs(M, plant)
        self.ldc = host.pop("ldc")
        self.d = {k: torch.from_numpy(v).to(device) for k, v in host.items()}
        self.result = torch.zeros(4, dtype=torch.int64, device=device)
        nbytes = max(int(self.lib.gpbo_acq_workspace_bytes()), _lib.MES_WORK_BYTES, _lib.CONS_WORK_BYTES, _lib.EHVI_WORK_BYTES)
        self.work = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        assert self.work.data_ptr() % 256 == 0

    def _out(self, dense):
        return self.torch.full((self.M,), SENTINEL, dtype=self.torch.float64, device=self.device) if dense else None

    def run(self, entry, par, dense):
        """{"sha": {output name: SHA-256}, "best_val": hex bits, "best_idx", "nan_count"} of one call."""
        L, lib, d, M = self.L, self.lib, self.d, self.M
        outs = {}
        self.result.fill_(-1)
        if entry == "acq":
            kind, p0, p1 = (L.ACQ_LCB, 4.0, 0.0) if par["kind"] == "lcb" else (L.ACQ_EI, -1.0, 0.015625)
            outs["acq"] = self._out(dense)
            L.call(lib.gpbo_acq_argmax_f64, d["mu"], d["sigma"], M, kind, p0, p1, OFFSET, outs["acq"], self.result, self.work,
                   int(lib.gpbo_acq_workspace_bytes()), None)
        elif entry == "mes":
            ys = -3.0 - np.arange(par["S"], dtype=np.float64) / 16.0
            outs["acq"] = self._out(dense)
            L.call(lib.gpbo_mes_acq_f64, d["mu"], d["sigma"], M, ys, par["S"], OFFSET, outs["acq"], self.result, self.work,
                   L.MES_WORK_BYTES, None)
        elif entry == "cons":
            C = par["C"]
            upper = 0.25 * np.arange(C, dtype=np.float64) - 0.5
            outs["val"], outs["feas"] = self._out(dense), self._out(dense)
            L.call(lib.gpbo_constrained_acq_f64, d["mu"], d["sigma"], M, L.CONS_BASE_IDS[par["base"]], -1.0, 0.015625,
                   d["cons_mu"] if C else None, d["cons_sigma"] if C else None, self.ldc if C else M, C, upper if C else None,
                   OFFSET, outs["val"], outs["feas"], self.result, self.work, L.CONS_WORK_BYTES, None)
        elif entry == "ehvi":
            F, r1, r2 = front(par["P"])
            outs["val"] = self._out(dense)
            L.call(lib.gpbo_ehvi_acq_f64, d["mu"], d["sigma"], d["mu2"], d["sigma2"], M, F if par["P"] else None, par["P"], r1, r2,
                   OFFSET, outs["val"], self.result, self.work, L.EHVI_WORK_BYTES, None)
        else:
            raise ValueError(entry)
        r = self.result.cpu().numpy()   # synchronises
        return {"sha": {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in outs.items() if v is not None},
                "best_val": struct.pack(">q", int(r[0])).hex(), "best_idx": int(r[1]), "nan_count": int(r[2])}


def record_all():
    got = {}
    for M, plant in size_variants():
        run = Runner(M, plant)
        for entry, par in cases():
            for dense in (True, False):
                got[case_id(entry, par, M, plant, dense)] = run.run(entry, par, dense)
    return got


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch  # noqa: F401  (its HIP runtime first)

    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    got = record_all()
    with open(path, "w") as f:   # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(got[k], sort_keys=True)}" for k in sorted(got)) + "\n}\n")
    print(f"wrote {len(got)} cases to {path}")
