"""The candidate tile of the direct contraction (k_contract16d: 64 rows a workgroup; k_contract16n: 32 or 16; csrc/kernels_posterior.hip,
DESIGN.md section 5.2''') on the device.  Rows of the contraction are independent and the order in which a row's columns are added
belongs to the column side, which the tile does not touch: predict(), every criterion value and every winner carry the SAME BITS at
all three tiles -- compared as bytes, no tolerance.  Shapes: N = 544 (three column groups, the last ragged; the model of
tests/prune_cases.py), N = 1040 (five, ragged), N = 768 (whole groups only); M around the tile edges, and 3001 rows in 1-MiB chunks
(several chunks, the last ragged; up to 32 rows there is no contraction launch at all and the setter must change nothing).  One pruned one-pass sweep (pilot = 192 rows) at every forced tile and at automatic; and with
BOGP_CONTRACT_DIRECT=0 (the LDS-staged kernel, a process of its own) the setter changes nothing."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import prune_cases as PC
from bogp import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_UCB, _lib.ACQ_MGFI
ACQ = [(EI, 0.0), (MGFI, 2.0), (UCB, 1.5)]
SIZES = (1, 15, 16, 17, 33, 63, 64, 65, 200)
TILES = (64, 32, 16)


def make_engine(N, kernel, ordinary, d=PC.DIM, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-5, 5, size=(N, d))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    eng = _lib.Engine(0)
    eng.set_train(X, y)
    eng.commit(kernel, _lib.MODE_NOISY, np.r_[np.full(d, 0.05), 0.01], PC.NOISE, ordinary, 0.0)
    return eng, float(y.min())


def outputs(eng, plugin):
    mu, mse = eng.predict()
    t_predict = eng.last_contract_tile()
    best, idx, vals = eng.sweep(ACQ, plugin, True, return_values=True)
    return (mu.tobytes(), mse.tobytes(), best.tobytes(), idx.tobytes(), vals.tobytes()), t_predict, eng.last_contract_tile()


@pytest.mark.parametrize("ordinary", [False, True], ids=["simple", "ordinary"])
@pytest.mark.parametrize("kernel", [_lib.KERNEL_MATERN52, _lib.KERNEL_SE], ids=["matern52", "se"])
@pytest.mark.parametrize("N", [544, 1040, 768])
def test_predict_and_sweep_values_have_the_same_bits_at_every_tile(monkeypatch, N, kernel, ordinary):
    eng, plugin = make_engine(N, kernel, ordinary)
    try:
        for M in SIZES + (3001,):
            if M == 3001:
                monkeypatch.setenv("BOGP_CHUNK_MB", "1")
            eng.upload_candidates(PC.candidates(seed=7 + M, M=M))
            runs = {}
            for tile in TILES:
                before = eng.last_contract_tile()
                eng.set_contract_tile(tile)
                runs[tile], t_predict, t_sweep = outputs(eng, plugin)
                # (up to 32 rows the posterior runs on the one-point kernels, sweep_small_batch: no contraction launch, nothing to report)
                assert (t_predict, t_sweep) == ((tile, tile) if M > 32 else (before, before)), (M, tile, t_predict, t_sweep)
            assert np.isfinite(np.frombuffer(runs[64][1])).all()
            for tile in (32, 16):
                assert runs[tile] == runs[64], "M = %d: %d-row tiles differ from 64-row tiles" % (M, tile)
            eng.set_contract_tile(0)
            auto, t_predict, t_sweep = outputs(eng, plugin)
            assert auto == runs[64] and t_predict in TILES and t_sweep in TILES
            if M == 3001:
                assert eng.last_timing()["n_chunks"] > 1
    finally:
        eng.close()


@pytest.mark.parametrize("ordinary", [False, True], ids=["simple", "ordinary"])
def test_pruned_one_pass_sweep_is_the_same_at_every_tile(monkeypatch, ordinary):
    """The sizes of tests/test_gpu_prune_onepass.py: 3001 rows in chunks of 192 = the pilot; UCB with multiplier 8 leaves about 175
    survivors for one round.  Pilot and round go through launch_contract at the forced tile."""
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")
    X, y, par, st = PC.model(ordinary)
    eng = _lib.Engine(0)
    try:
        eng.set_train(X, y)
        eng.commit(PC.KERNEL, _lib.MODE_NOISY, par, PC.NOISE, ordinary, 0.0)
        eng.upload_candidates(PC.candidates())
        acq = [(UCB, 8.0), (UCB, 0.5)]
        runs = []
        for tile in (64, 32, 16, 0):
            eng.set_contract_tile(tile)
            v, i = eng.sweep(acq, float(y.min()), True)
            runs.append((v.tobytes(), i.tobytes(), eng.last_prune_path(), eng.last_contracted_rows()))
            if tile:
                assert eng.last_contract_tile() == tile
        assert runs[0][2][0] == _lib.PRUNE_PATH_ONEPASS and runs[0][2][1] > 0 and runs[0][3] == PC.CHUNK_ROWS + runs[0][2][1]
        for r in runs[1:]:
            assert r == runs[0]
        eng.set_prune(False)
        eng.set_contract_tile(64)
        v, i = eng.sweep(acq, float(y.min()), True)
        assert (v.tobytes(), i.tobytes()) == runs[0][:2]
    finally:
        eng.close()


def test_the_setter_refuses_other_values_on_the_device():
    eng, _ = make_engine(544, _lib.KERNEL_MATERN52, False)
    try:
        assert eng.last_contract_tile() == 64
        for bad in (-1, 1, 8, 48, 128):
            with pytest.raises(ValueError):
                eng.set_contract_tile(bad)
            with pytest.raises(_lib.BogpError):  # the library's own check, behind the binding's
                eng._check(eng._lib.bogp_set_contract_tile(eng._h, bad))
        assert eng.last_contract_tile() == 64
    finally:
        eng.close()


def tile_digests():
    """{tile set: [sha1 over predict() and the sweep's values, last_contract_tile()]} for automatic and the three forced tiles"""
    import hashlib

    out = {}
    eng, plugin = make_engine(544, _lib.KERNEL_MATERN52, True)
    try:
        eng.upload_candidates(PC.candidates(seed=3, M=777))
        for tile in (0, 16, 32, 64):
            eng.set_contract_tile(tile)
            h = hashlib.sha1()
            for a in outputs(eng, plugin)[0]:
                h.update(a)
            out[str(tile)] = [h.hexdigest(), eng.last_contract_tile()]
    finally:
        eng.close()
    return out


CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from test_gpu_contract_tile import tile_digests
print("RESULT " + json.dumps(tile_digests()))
'''


def test_the_lds_staged_kernel_ignores_the_setter_and_gives_the_default_bits():
    e = dict(os.environ)
    e["BOGP_CONTRACT_DIRECT"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=600)  # fmt: skip
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    staged = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    direct = tile_digests()
    assert {v[1] for v in staged.values()} == {64}, staged
    assert [direct[t][1] for t in ("16", "32", "64")] == [16, 32, 64], direct
    assert len({v[0] for v in staged.values()} | {v[0] for v in direct.values()}) == 1, (staged, direct)
