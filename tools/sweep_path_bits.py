#!/usr/bin/env python3
"""Digests of everything the sweep's host paths return, one child process per case (the library reads its switches once): a sha1
over every array of the call plus last_prune_path, last_contracted_rows and n_chunks.  Two builds agree on a host-side refactor
exactly when their listings agree line for line:

    python tools/sweep_path_bits.py                    > pr.txt       # the tree this file sits in
    python tools/sweep_path_bits.py --root ../parent   > parent.txt   # another checkout with its own libbogp.so

The cases are the smallest that reach each branch of run_sweep (csrc/bogp_api_sweep.hip): the <= 32-row batch, the one-launch
sweep, the chunk loop with its trend variants / two streams / lazy upload, the queued sweep, both pruned flows with their
fall-backs, EHVI, the believer batches of the four families (several chunks, one resident chunk, a guarded pivot in front of step 0),
Thompson batches, the lifted sweep and Thompson batches under modelled constraints.  Needs an MI355X."""
import argparse
import collections
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def digest(*arrs):
    import numpy as np

    h = hashlib.sha1()
    for a in arrs:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def report(eng, name, *arrs):
    path, surv, rounds = eng.last_prune_path()
    print("BITS %-34s %s path=%d survivors=%d rounds=%d contracted=%d n_chunks=%d"
          % (name, digest(*arrs), path, surv, rounds, eng.last_contracted_rows(), eng.last_timing()["n_chunks"]))  # fmt: skip


def smooth_model(_lib, rng, N, d, kernel=3, trend=0, targets=1):  # (several targets: a fixed constant trend, the only one they take)
    import numpy as np

    X = rng.uniform(-5, 5, (N, d))
    y = np.stack([np.sum(np.sin(X + t), axis=1) for t in range(targets)], axis=1)
    y = (y - y.mean(axis=0)) / y.std(axis=0) + 0.2 * rng.standard_normal((N, targets))
    eng = _lib.Engine(0)
    eng.set_train(X, y)
    eng.commit(kernel, 1, np.r_[np.full(d, 0.3 / d), 0.9], 1e-4, targets == 1, 0.0, trend=trend)
    return eng, X, y


def predict_and_sweep(eng, name, y, with_mean_only=True):
    mu, mse = eng.predict()
    report(eng, name + "/predict", mu, mse)
    if with_mean_only:
        mu0, _ = eng.predict(eval_MSE=False)
        report(eng, name + "/predict-mean", mu0)
    best, idx, vals = eng.sweep([(0, 0.0), (3, 2.0)], float(y.min()), True, return_values=True)
    report(eng, name + "/sweep-q2-values", best, idx, vals)


def case_small(_lib, np, rng, what):
    if what.startswith("batch"):  # N = 600: M = 7 and 32 take the small batch, 33 the chunk loop in one chunk
        eng, X, y = smooth_model(_lib, rng, 600, 3)
        for M in (7, 32, 33):
            eng.upload_candidates(rng.uniform(-5, 5, (M, 3)))
            predict_and_sweep(eng, "N600-M%d" % M, y)
    else:  # one launch: N = 300, M = 1000 (neither a multiple of 16 nor of 64); also under BOGP_SMALL_STAMPS=1
        eng, X, y = smooth_model(_lib, rng, 300, 4, kernel=0)
        eng.upload_candidates(rng.uniform(-5, 5, (1000, 4)))
        predict_and_sweep(eng, "one-launch", y)
    eng.close()


def case_chunked(_lib, np, rng, what):
    """The `sweep` script of tests/test_gpu_switches.py (N = 700, M = 9000, BOGP_CHUNK_MB=8: seven chunks, the last one 168 rows;
    constant / linear / quadratic trend), plus a mean-only predict on each model."""
    for trend, d in ((0, 5), (1, 5), (2, 8)):
        N, M = 700, 9000
        X = rng.uniform(-5, 5, (N, d)); y = np.sum(np.sin(X), axis=1); y = ((y - y.mean()) / y.std() + 0.2 * rng.standard_normal(N)).reshape(-1, 1)  # noqa: E702
        eng = _lib.Engine(0); eng.set_train(X, y)  # noqa: E702
        eng.commit(3, 1, np.r_[np.full(d, 0.3 / d), 0.9], 1e-4, True, 0.0, trend=trend)
        Xs = rng.uniform(-5, 5, (M, d))
        lazy = what == "lazy"
        eng.upload_candidates(Xs, lazy=lazy)
        mu, mse = eng.predict()
        report(eng, "trend%d/predict" % trend, mu, mse)
        if lazy:
            eng.upload_candidates(Xs, lazy=True)
        best, idx, vals = eng.sweep([(0, 0.0), (3, 2.0)], float(y.min()), True, return_values=True)
        report(eng, "trend%d/sweep-q2-values" % trend, best, idx, vals)
        if lazy:
            eng.upload_candidates(Xs, lazy=True)
        mu0, _ = eng.predict(eval_MSE=False)
        report(eng, "trend%d/predict-mean" % trend, mu0)
        if lazy:  # a sweep without value outputs over lazily uploaded rows: the per-chunk pruned flow beside the copies
            eng.upload_candidates(Xs, lazy=True)
            best, idx = eng.sweep([(0, 0.0), (3, 2.0)], float(y.min()), True)
            report(eng, "trend%d/sweep-q2" % trend, best, idx)
        eng.close()


def case_pruned(_lib, np, rng, what):
    """Model and candidates of tests/prune_cases.py (N = 544, d = 3, M = 3001, BOGP_CHUNK_MB=1) with the UCB multipliers of
    tests/test_gpu_prune_onepass.py: one / two / three rounds, the pilot-share route to the per-chunk path, the forced segment
    fall-back, the queued sweep with the one-rank exchange; and M = 13005 at BOGP_CHUNK_MB=24, chunk 0 larger than the pilot."""
    import prune_cases as PC
    from oracle import gp_oracle as O

    UCB = _lib.ACQ_UCB
    for ordinary in (False, True):
        X, y, par, st = PC.model(ordinary)
        eng = _lib.Engine(0)
        eng.set_train(X, y)
        eng.commit(PC.KERNEL, _lib.MODE_NOISY, par, PC.NOISE, ordinary, 0.0)
        pl = float(y.min())
        tag = "ok" if ordinary else "sk"
        if what == "large":
            acq = [(_lib.ACQ_MGFI, 2.0), (_lib.ACQ_EI, 0.0)]
            for where in (4000, 13002):
                eng.upload_candidates(PC.place_winner(st, PC.candidates(seed=9, M=13005), acq, pl, where))
                for mode in (True, "chunks", False):
                    eng.set_prune(mode)
                    report(eng, "%s/M13005-w%d/prune-%s" % (tag, where, mode), *eng.sweep(acq, pl, True))
            eng.close()
            continue
        Xs = PC.candidates()
        eng.upload_candidates(Xs)
        for alpha in (0.5, 8.0, 10.0, 15.0, 20.0, 50.0):  # one, one, two, three rounds; 20 and 50: what the pilot share decides
            for mode in (True, "chunks"):
                eng.set_prune(mode)
                report(eng, "%s/ucb%g/prune-%s" % (tag, alpha, mode), *eng.sweep([(UCB, alpha)], pl, True))
        # forced segment fall-back: the pilot holds the winner and the 191 rows with the lowest bounds (UCB, alpha = 30)
        mu, mse, sd_ub = PC.oracle_rows(st, Xs)
        s2 = float(st.sigma2[0])
        w = int(np.argmax(O.acquisition(UCB, 30.0, mu, mse, pl, s2, True)))
        b = PC.upper_bounds(UCB, 30.0, mu, sd_ub, pl, s2)
        head = np.array([w] + [int(r) for r in np.argsort(b, kind="stable") if r != w][: PC.CHUNK_ROWS - 1])
        eng.upload_candidates(Xs[np.r_[head, np.setdiff1d(np.arange(len(Xs)), head)]])
        for mode in (True, "chunks"):
            eng.set_prune(mode)
            report(eng, "%s/fallback-ucb30/prune-%s" % (tag, mode), *eng.sweep([(UCB, 30.0)], pl, True))
        if not ordinary:  # queued: NULL best_val, then the one-rank exchange
            from bogp import distributed

            acq = [(UCB, 8.0), (UCB, 0.5)]
            Xw = PC.place_winner(st, Xs, acq, pl, 2222)
            eng.upload_candidates(Xw)
            eng.set_prune(True)
            assert distributed.init_engine_comm(eng) == (0, 1)
            assert eng.sweep(acq, pl, True, local_result=False) is None
            report(eng, "sk/queued-onepass/exchange", *eng.exchange_argmax(len(acq), 1_000_000, True))
            eng.upload_candidates(Xw, lazy=True)
            assert eng.sweep(acq, pl, True, local_result=False) is None
            report(eng, "sk/queued-lazy/exchange", *eng.exchange_argmax(len(acq), 0, True))
        eng.close()


def case_batches(_lib, np, rng, what):
    N, M = 700, 3000
    if what == "ehvi":  # m = 2 targets, with and without the moment outputs; the believer's EHVI form, q = 2
        eng, X, y = smooth_model(_lib, rng, N, 4, targets=2)
        eng.upload_candidates(rng.uniform(-5, 5, (M, 4)))
        lower = np.array([[-3.0, -3.0], [-0.5, -3.0], [0.4, -3.0]])
        upper = np.array([[-0.5, np.inf], [0.4, 0.3], [np.inf, -0.6]])
        report(eng, "ehvi/values", *eng.sweep_ehvi(lower, upper, k=1, return_values=True))
        report(eng, "ehvi/values+moments", *eng.sweep_ehvi(lower, upper, k=3, return_values=True, return_moments=True))
        out = eng.sweep_believer_ehvi(np.array([[-0.5, 0.3], [0.4, -0.6]]), np.array([-3.0, -3.0]), 2, return_values=True)
        report(eng, "believer-ehvi/q2", *[out[k] for k in sorted(out)])
        pend = rng.uniform(-5, 5, (1, 4))
        out = eng.sweep_believer_ehvi(np.array([[-0.5, 0.3], [0.4, -0.6]]), np.array([-3.0, -3.0]), 2, pending=pend, return_values=True)
        report(eng, "believer-ehvi/q2-pending", *[out[k] for k in sorted(out)])
    elif what == "believer":  # q = 3, without and with a pending point
        eng, X, y = smooth_model(_lib, rng, N, 4)
        eng.upload_candidates(rng.uniform(-5, 5, (M, 4)))
        acq = [(0, 0.0), (3, 2.0), (2, 1.5)]
        out = eng.sweep_believer(acq, float(y.min()), True, return_values=True)
        report(eng, "believer/q3", *[out[k] for k in sorted(out)])
        out = eng.sweep_believer(acq, float(y.min()), True, pending=rng.uniform(-5, 5, (2, 4)), return_values=True)
        report(eng, "believer/q3-pending", *[out[k] for k in sorted(out)])
    elif what == "believer-constrained":  # m = 3: two constraints at inner quantiles; q = 3 with a feasibility-only step, without and with pending points
        eng, X, y = smooth_model(_lib, rng, N, 4, targets=3)
        eng.upload_candidates(rng.uniform(-5, 5, (M, 4)))
        lo, hi = np.quantile(y[:, 1:], [0.25, 0.75], axis=0)
        acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_NONE, 0.0), (_lib.ACQ_MGFI, 2.0)]
        out = eng.sweep_believer_constrained(acq, float(y[:, 0].min()), True, lo, hi, return_values=True)
        report(eng, "believer-constrained/q3", *[out[k] for k in sorted(out)])
        out = eng.sweep_believer_constrained(acq, float(y[:, 0].min()), True, lo, hi, pending=rng.uniform(-5, 5, (2, 4)), return_values=True)
        report(eng, "believer-constrained/q3-pending", *[out[k] for k in sorted(out)])
    elif what == "believer-ehvi-constrained":  # m = 2 objectives + 1 constraint at inner quantiles; q = 3 over a front, then feasibility only
        eng, X, y = smooth_model(_lib, rng, N, 4, targets=3)
        eng.upload_candidates(rng.uniform(-5, 5, (M, 4)))
        lo, hi = np.quantile(y[:, 2:], [0.25, 0.75], axis=0)
        ok = np.all((y[:, 2:] >= lo) & (y[:, 2:] <= hi), axis=1)
        rp = y[:, :2].min(axis=0) - 0.1
        out = eng.sweep_believer_ehvi_constrained(y[ok, :2], rp, 3, lo, hi, return_values=True)
        report(eng, "believer-ehvi-constrained/q3", *[out[k] for k in sorted(out)])
        pend = rng.uniform(-5, 5, (2, 4))
        out = eng.sweep_believer_ehvi_constrained(y[ok, :2], rp, 3, lo, hi, pending=pend, return_values=True)
        report(eng, "believer-ehvi-constrained/q3-pending", *[out[k] for k in sorted(out)])
        out = eng.sweep_believer_ehvi_constrained(None, rp, 3, lo, hi, pending=pend, feasibility_only=True, return_values=True)
        report(eng, "believer-ehvi-constrained/q3-pending-feasibility-only", *[out[k] for k in sorted(out)])
    elif what == "thompson":  # conditioned, L = 64, q = 2, k = 1 and k = 3 (a noiseless model: the only mode it takes)
        d = 4
        X = rng.uniform(-2, 2, (N, d))
        y = 2 * np.sin(X @ rng.normal(size=d) / np.sqrt(d)) + 0.1 * rng.normal(size=N)
        nn = 4.0 / N ** (1.0 / d)
        eng = _lib.Engine(0)
        eng.set_train(X, y.reshape(-1, 1))
        eng.commit(3, _lib.MODE_NOISELESS, np.full(d, 1.0 / (d * nn * nn)), 0.0, True, 0.3)
        eng.upload_candidates(rng.uniform(-2.2, 2.2, (M, d)))
        Draw = collections.namedtuple("Draw", "omega phase weights eps")
        dr = Draw(rng.normal(size=(64, d)), rng.uniform(0, 2 * np.pi, 64), rng.normal(size=(64, 2)), rng.normal(size=(N, 2)))
        for k in (1, 3):
            out = eng.sweep_thompson(dr, minimize=True, k=k, conditioned=True, return_values=k == 3)
            report(eng, "thompson/k%d" % k, out["best_val"], out["best_idx"], out["best_x"], out["coef"][0], out["coef"][1], out.get("paths"))
    elif what == "thompson-constrained":  # m = 3 joint paths, q = 5 members (15 columns), L = 64, k = 1 and k = 3
        d, m, q = 4, 3, 5
        X = rng.uniform(-2, 2, (N, d))
        Y = np.column_stack([2 * np.sin(X @ rng.normal(size=d) / np.sqrt(d)) + 0.1 * rng.normal(size=N) for _ in range(m)])
        nn = 4.0 / N ** (1.0 / d)
        eng = _lib.Engine(0)
        eng.set_train(X, Y)
        eng.commit(3, _lib.MODE_NOISELESS, np.full(d, 1.0 / (d * nn * nn)), 0.0, False, 0.3)
        eng.upload_candidates(rng.uniform(-2.2, 2.2, (M, d)))
        Draw = collections.namedtuple("Draw", "omega phase weights eps")
        dr = Draw(rng.normal(size=(64, d)), rng.uniform(0, 2 * np.pi, 64), rng.normal(size=(64, q * m)), rng.normal(size=(N, q * m)))
        lo, hi = np.full(m - 1, -np.inf), np.median(Y[:, 1:], axis=0)
        for k in (1, 3):
            out = eng.sweep_thompson_constrained(dr, q, lo, hi, minimize=True, k=k, return_values=k == 3)
            report(eng, "thompson-constrained/k%d" % k, out["best_val"], out["best_idx"], out["best_x"], out["coef"], out.get("paths"))
    else:  # one lifted sweep: r = 3 model, D = 5 box, part of the rows infeasible
        eng, X, y = smooth_model(_lib, rng, N, 3)
        eng.upload_candidates(rng.uniform(-5, 5, (M, 3)))
        A = np.linalg.qr(rng.normal(size=(5, 3)))[0].T
        eng.set_lift(A, np.zeros(5), None, -3.0 * np.ones(5), 3.0 * np.ones(5))
        best, idx, nf, vals, pen = eng.lift_sweep_topk([(0, 0.0), (3, 2.0)], float(y.min()), True, k=3, return_values=True, return_penalty=True)
        assert 0 < nf < M, nf
        report(eng, "lift/topk3 (%d feasible)" % nf, best, idx, vals, pen)
    eng.close()


def case_guard(_lib, np, rng, what):
    """The guarded pivot in front of step 0, as the test_pivot_guard tests construct it: the last pending point is a training
    row of a noiseless model (pivot <= 1e-12), the plugin / front held fixed.  One, two and three targets (the three read as objective + constraints and as two objectives + one constraint)."""
    N, M, d = 700, 3000, 4
    X = rng.uniform(-2, 2, (N, d))
    Y = np.sin(X @ rng.normal(size=(d, 3))) * (1.0 + np.arange(3)) + 0.3 * rng.normal(size=(N, 3))
    Xs = rng.uniform(-2.2, 2.2, (M, d))
    pend = np.vstack([rng.uniform(-2, 2, (1, d)), X[5]])
    eng = _lib.Engine(0)

    def commit(m):
        eng.set_train(X, Y[:, :m])
        eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, np.array([1.0, 0.8, 1.3, 1.1]) * 8.0, 0.0, m == 1, 0.1)
        eng.upload_candidates(Xs)

    def guarded(name, out):
        assert out["pivots"][1] <= 1e-12, out["pivots"]
        report(eng, name, *[out[k] for k in sorted(out)])

    commit(1)
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 2.0), (_lib.ACQ_EPSILON_PI, 1.5)]
    guarded("believer/q3-guarded", eng.sweep_believer(acq, float(Y[:, 0].min()), True, pending=pend, believe_plugin=False, return_values=True))
    commit(2)
    front, rp = np.array([[-0.5, 0.3], [0.4, -0.6]]), np.array([-3.0, -3.0])
    guarded("believer-ehvi/q2-guarded", eng.sweep_believer_ehvi(front, rp, 2, pending=pend, believe_front=False, return_values=True))
    commit(3)
    lo, hi = np.quantile(Y[:, 1:], [0.25, 0.75], axis=0)
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_NONE, 0.0), (_lib.ACQ_MGFI, 2.0)]
    guarded("believer-constrained/q3-guarded",
            eng.sweep_believer_constrained(acq, float(Y[:, 0].min()), True, lo, hi, pending=pend, believe_plugin=False, return_values=True))  # fmt: skip
    guarded("believer-ehvi-constrained/q2-guarded",  # the same three-target model read as two objectives and one constraint
            eng.sweep_believer_ehvi_constrained(front, rp, 2, lo[1:], hi[1:], pending=pend, believe_front=False, return_values=True))  # fmt: skip
    eng.close()


# name -> (function, argument, environment)
CASES = collections.OrderedDict([
    ("small-batch", (case_small, "batch", {})),
    ("one-launch", (case_small, "launch", {})),
    ("one-launch-stamps", (case_small, "launch", {"BOGP_SMALL_STAMPS": "1"})),
    ("chunked", (case_chunked, "", {"BOGP_CHUNK_MB": "8"})),
    ("chunked-overlap", (case_chunked, "", {"BOGP_CHUNK_MB": "8", "BOGP_OVERLAP": "1"})),
    ("chunked-lazy", (case_chunked, "lazy", {"BOGP_CHUNK_MB": "8"})),
    ("pruned", (case_pruned, "", {"BOGP_CHUNK_MB": "1"})),
    ("pruned-large", (case_pruned, "large", {"BOGP_CHUNK_MB": "24"})),
    ("ehvi", (case_batches, "ehvi", {"BOGP_CHUNK_MB": "8"})),
    ("believer", (case_batches, "believer", {"BOGP_CHUNK_MB": "8"})),
    ("believer-constrained", (case_batches, "believer-constrained", {"BOGP_CHUNK_MB": "8"})),
    ("believer-ehvi-constrained", (case_batches, "believer-ehvi-constrained", {"BOGP_CHUNK_MB": "8"})),
    ("ehvi-one-chunk", (case_batches, "ehvi", {})),  # the believers again with every candidate in one chunk: the producer runs once
    ("believer-one-chunk", (case_batches, "believer", {})),
    ("believer-constrained-one-chunk", (case_batches, "believer-constrained", {})),
    ("believer-ehvi-constrained-one-chunk", (case_batches, "believer-ehvi-constrained", {})),
    ("believer-guard", (case_guard, "", {"BOGP_CHUNK_MB": "8"})),
    ("believer-guard-one-chunk", (case_guard, "", {})),
    ("thompson", (case_batches, "thompson", {"BOGP_CHUNK_MB": "8"})),
    ("lift", (case_batches, "lift", {"BOGP_CHUNK_MB": "8"})),
    ("thompson-constrained", (case_batches, "thompson-constrained", {"BOGP_CHUNK_MB": "8"})),  # (behind the older cases: their lines keep their place)
])  # fmt: skip


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package and library are loaded")
    ap.add_argument("--case", help="run this case in this process (what the driver starts)")
    ap.add_argument("--only", nargs="*", help="driver: these cases only")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.case:
        sys.path[:0] = [root, os.path.join(root, "tests")]
        import numpy as np

        from bogp import _lib

        assert os.path.dirname(os.path.abspath(_lib.__file__)).startswith(root), _lib.__file__
        fn, arg, _ = CASES[args.case]
        fn(_lib, np, np.random.default_rng(12), arg)
        return 0
    for name in args.only or CASES:
        env = dict(os.environ)
        for k in ("BOGP_CHUNK_MB", "BOGP_OVERLAP", "BOGP_SMALL_STAMPS"):
            env.pop(k, None)
        env.update(CASES[name][2])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--case", name], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            print("FAILED %s (exit %d)\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
            return 1
        for ln in r.stdout.splitlines():
            if ln.startswith("BITS "):
                print("%-18s %s" % (name, ln[5:]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
