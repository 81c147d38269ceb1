"""How often does a trip of the box active set (gi_box_st) hold a partial step?

A NumPy restatement of the method on the config-2 instances of bench.py (slot
0 of the rank-0 seed: N = 20, |u| <= 1, x0 ~ U(-10, 10)^2), grouped as
mpc_group_kernel packs them: four consecutive instances per wave, every group
starting its trips together, a wave running as many trips as its slowest
group.  Records, under profiles/:
  iterations per QP (mean, max), partial steps per QP (histogram),
  trips per wave, and the share of trips with a partial step in any group --
  the trips that take the general path; all others take the full-step trip.

    python tools/gi_partial_share.py [--batch 4096] [--check DIR]

--check DIR: the directory of `bench.py --config 2 --dump-outputs DIR` run with
`--steps K` such that (K - 1) % 8 == 0 (the dump is the last step's slot):
the model's per-instance iteration counts must equal status_iters.npy.
The warm-started steps of the config-2 loop are not restated here (they need
the loop's shifted active set and its release scan).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import condense as oc  # noqa: E402

KB = 5  # key bits at NMAX = 20


def clear(v):
    u = np.array([v], dtype=np.float64).view(np.uint64)
    u &= ~np.uint64((1 << KB) - 1)
    return float(u.view(np.float64)[0])


def gi_trips(Minv, f, lb, ub, tol=1e-12):
    """One bool per trip (True: partial step) of the cold-started active set."""
    n = f.size
    M = Minv.copy()
    st = np.zeros(n, int)
    mu = np.zeros(n)
    z = M @ f
    trips = []

    def sweep(k, sigma):
        d = M[k, k]
        col, row = M[:, k].copy(), M[k, :].copy()
        M[:] = M - np.outer(col, row) / d
        M[k, :] = sigma * row / d
        M[:, k] = sigma * col / d
        M[k, k] = -1.0 / d

    while True:
        v = np.fmax((lb - z) / (1 + np.abs(lb)), (z - ub) / (1 + np.abs(ub)))
        v = np.where(st == 0, v, -np.inf)
        p = int(np.argmax(v))
        if not clear(v[p]) > tol:
            return trips
        side = 1 if z[p] < lb[p] else 2
        tgt = lb[p] if side == 1 else ub[p]
        zp, gp = z[p], 0.0
        while True:
            assert len(trips) < 200
            c, rm = M[:, p].copy(), 1.0 / M[p, p]
            sgn = 1.0 if tgt > zp else -1.0
            t2 = abs(tgt - zp)
            cs = c * rm
            dmu = np.where(st == 1, -cs, np.where(st == 2, cs, 0.0)) * sgn
            cand = (st != 0) & (dmu < 0)
            t = np.where(cand, -mu / np.where(cand, dmu, 1.0), np.inf)
            k = int(np.argmin(t))
            ti = clear(t[k]) if np.isfinite(t[k]) else np.inf
            partial = ti < t2
            trips.append(bool(partial))
            s = ti if partial else t2
            z = np.where(st == 0, z + sgn * s * cs, z)
            mu = mu + s * dmu
            gp -= sgn * s * rm
            zp += sgn * s
            if partial:
                sweep(k, 1.0)
                st[k], mu[k] = 0, 0.0
            else:
                sweep(p, -1.0)
                st[p], z[p], mu[p] = side, tgt, (gp if side == 1 else -gp)
                break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--check", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gi_partial_share.json"))
    a = ap.parse_args()
    ts, N = 0.5, 20
    A = np.array([[1.0, ts], [0.0, 1.0]])
    B = np.array([[0.0], [-ts]])
    C = np.array([[1.0], [-2.0 / 3.0]])
    Q = C @ C.T + 1e-3 * np.eye(2)
    R = np.array([[0.1]])
    rng = np.random.default_rng(20261015 + 2)          # bench.py Config2, rank 0
    X0 = rng.uniform(-10.0, 10.0, size=(8, 4096, 2))[0][:a.batch]
    cd = oc.condense(A, B, Q, R, Q, N)
    Minv = -np.linalg.inv(cd["H"])
    lb, ub = -np.ones(N), np.ones(N)
    trips = [gi_trips(Minv, cd["F"] @ x0, lb, ub) for x0 in X0]
    iters = np.array([len(t) for t in trips])
    parts = np.array([sum(t) for t in trips])
    wave_trips, wave_partial = [], []
    for w in range(0, len(trips), 4):
        grp = trips[w:w + 4]
        nt = max(len(t) for t in grp)
        wave_trips.append(nt)
        wave_partial.append(sum(any(len(t) > i and t[i] for t in grp) for i in range(nt)))
    wave_trips, wave_partial = np.array(wave_trips), np.array(wave_partial)
    res = {
        "instances": int(len(trips)),
        "iterations_mean": float(iters.mean()), "iterations_max": int(iters.max()),
        "partial_steps_per_qp_hist": {str(k): int((parts == k).sum()) for k in np.unique(parts)},
        "trips_per_wave_mean": float(wave_trips.mean()),
        "partial_trips_per_wave_mean": float(wave_partial.mean()),
        "share_of_trips_with_a_partial_step": float(wave_partial.sum() / wave_trips.sum()),
    }
    if a.check:
        dev = np.load(os.path.join(a.check, "status_iters.npy")).astype(int)[:a.batch]
        res["device_iterations_equal"] = bool(np.array_equal(dev, iters))
        res["device_iterations_differing"] = int((dev != iters).sum())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
