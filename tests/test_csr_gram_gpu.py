"""``srml_csr_gram_*`` / ``srml_csr_xty_*`` (csrc/csr_gram.hip) and the sparse LinearRegression / PCA
fits on the device: the cases, oracle and bounds of ``tests/test_csr_gram.py``, at both tile widths."""
import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from test_csr_gram import C, R, SHAPES, T, U, check, det, fit_and_check, make, to_csr  # noqa: F401  (det: fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tile", [T, 128 if T == 64 else 64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_gram_and_xty_meet_the_contract(gpu_device, name, dtype, tile, det):
    S = make(name, dtype, tile=tile)  # a dense row's segment is `tile` long: past the chunk C at 128
    assert max(T, 128) > C
    A = to_csr(S, gpu_device)
    G = ops.csr_gram(A, tile=tile)
    print("error / bound", name, dtype.__name__, tile, det, check(G, S, det))
    if det:
        assert torch.equal(G, ops.csr_gram(A, tile=tile))
    for yt in (np.float32, np.float64):
        y = np.random.default_rng(1).standard_normal(S.shape[0]).astype(yt)
        Xd = np.asarray(S.todense(), dtype=np.float64)
        got = ops.csr_xty(A, torch.from_numpy(y).to(gpu_device)).cpu().numpy()
        assert (np.abs(got - Xd.T @ y) <= (S.shape[0] + 2) * U * (np.abs(Xd).T @ np.abs(y.astype(np.float64)))).all()


def test_small_integers_and_row_blocks_are_exact(gpu_device, det):
    S = make("three_tiles", np.float32, integers=True)
    check(ops.csr_gram(to_csr(S, gpu_device)), S, det, exact=True)
    lo, hi = R // 2, 2 * R + 3  # a row block with its absolute offsets
    check(ops.csr_gram(to_csr(S, gpu_device, lo, hi)), S[lo:hi], det, exact=True)


def test_three_row_chunks_add_up(gpu_device, monkeypatch, det):
    S = make("three_tiles", np.float32)
    m, W = S.shape[0], -(-S.shape[1] // T)
    launches, real = [], ops.native.call_status
    monkeypatch.setattr(ops.native, "call_status", lambda n, *a: (launches.append(n), real(n, *a))[1])
    monkeypatch.setattr(ops, "_CSR_GRAM_WIN_BYTES", 4 * (W + 1) * -(-m // 3))
    check(ops.csr_gram(to_csr(S, gpu_device)), S, det)
    assert [n for n in launches if n == "srml_csr_gram_f32"] == ["srml_csr_gram_f32"] * 3


@pytest.mark.parametrize("workers", [1, 2])
def test_sparse_fits_match_numpy(gpu_device, workers, monkeypatch):
    monkeypatch.delenv("SRML_FORCE_CPU", raising=False)
    fit_and_check(workers, monkeypatch)
