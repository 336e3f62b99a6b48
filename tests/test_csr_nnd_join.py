"""``ops.csr_nnd_join`` (the NN-descent join on CSR rows) against the literal oracle of
``csr_nnd_cases``: every case on the torch form (CPU) and, marked ``gpu``, on the kernel; then the
checker itself against injected faults."""
import pytest
import torch

import csr_knn_cases as C
import csr_nnd_cases as J
from spark_rapids_ml_nai_amd import ops

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]


def test_exported_constants_are_the_kernels():
    """The cap cases of ``csr_nnd_cases`` are derived from these: they must be the kernel's own."""
    lib = ops.native.lib()
    got = tuple(int(lib.srml_csr_nnd_config(i)) for i in range(3))
    assert got == (ops.CSR_NND_CAND_CAP, ops.CSR_NND_LDS_CAP, ops.CSR_NND_KMAX) == (J.CAP, J.LDS, 64)
    assert int(lib.srml_csr_nnd_config(3)) == -1
    assert J.CAP & (J.CAP - 1) == 0  # the in-LDS sort needs a power of two
    assert J.LDS * 8 + J.CAP * 12 <= 64 * 1024  # staged row + slots + keys fit a workgroup's LDS


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("name", sorted(J.SPEC))
def test_join_matches_the_oracle(dev, name):
    case = J.case(name)
    keys, ids = J.run(case, dev)
    assert keys.device.type == dev and ids.device.type == dev
    J.check_join(case, keys, ids)
    keys2, ids2 = J.run(case, dev)  # a second call repeats bit for bit
    assert torch.equal(keys.view(torch.int32), keys2.view(torch.int32)) and torch.equal(ids, ids2)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("name", ["n65_lds_cap", "n257_padded_k64", "n600_random_k15_hellinger",
                                  "n600_star_k15_jaccard"])
def test_row_block_at_an_offset_equals_the_full_call(dev, name):
    case = J.case(name)
    keys, ids = J.run(case, dev)
    for r0, r1 in ((1, 2), (3, 9), (case.N - 7, case.N)):
        kb, ib = J.run(case, dev, r0, r1)
        J.check_join(case, kb, ib, r0, r1)
        assert torch.equal(kb.view(torch.int32), keys[r0:r1].view(torch.int32)) and torch.equal(ib, ids[r0:r1])


def test_case_table_covers_the_kernel_edges():
    """The shapes the table is meant to hold: the candidate cap and the LDS cap on both sides, every
    start graph, padded outputs, fan-outs wider than the list."""
    spec = J.SPEC
    total = sorted(s[7] + min(s[9][0], s[7]) * min(s[9][1], s[7]) + s[9][2] for s in spec.values())
    assert {J.CAP - 1, J.CAP, J.CAP + 1} <= set(total)
    assert {s[6] for s in spec.values()} == {"random", "ring", "star", "padded", "dups"}
    assert {s[2] for s in spec.values()} == {2, 4, 65, 257, 600}
    assert {1, 5, 15, 33, 64} <= {s[8] for s in spec.values()}
    assert any(s[8] >= s[2] for s in spec.values()) and any(s[9][0] > s[7] for s in spec.values())
    assert {J.LDS - 1, J.LDS, J.LDS + 1} <= set(J.LONG.values()) and 2100 in J.LONG.values()
    ring = J.case("n65_ring_k15")
    assert bool(((ring.off[1:] - ring.off[:-1]) == 15).all())  # every reverse list has exactly k entries
    star = J.case("n600_star_k15_jaccard")
    assert int(star.off[1]) - int(star.off[0]) == 600 > star.R and int(star.off[-1]) - int(star.off[1]) == 0
    dups = J.case("n65_dups_k5_jaccard")
    assert bool((dups.pos == dups.pos[:, :1]).all())
    lds = J.case("n65_lds_cap")
    nnz = (lds.A.indptr[1:] - lds.A.indptr[:-1]).tolist()
    assert nnz[1] == 0 and [nnz[r] for r in (3, 4, 6, 8)] == [J.LDS - 1, J.LDS, J.LDS + 1, lds.A.shape[1]]


def test_refusals():
    case = J.case("n65_ring_k15")
    P = ops.csr_prepare(case.A, "sqeuclidean")
    with pytest.raises(ValueError, match="graph must be"):
        ops.csr_nnd_join(P, P, case.pos[:10], case.perm, case.off, 15, 8, 8, 16, "sqeuclidean")
    with pytest.raises(ValueError, match="outside the graph"):
        ops.csr_nnd_join(P.rows(0, 10), P, case.pos, case.perm, case.off, 15, 8, 8, 16, "sqeuclidean", row0=60)
    with pytest.raises(ValueError, match="needs perm"):
        ops.csr_nnd_join(P, P, case.pos, None, None, 15, 8, 8, 16, "sqeuclidean")
    with pytest.raises(ValueError, match="prepared for"):
        ops.csr_nnd_join(P, P, case.pos, case.perm, case.off, 15, 8, 8, 16, "jaccard")


# ---- the checker against injected faults (CPU) ----------------------------------------------
def _fails(case, keys, ids, match):
    with pytest.raises(AssertionError, match=match):
        J.check_join(case, keys, ids)


def test_checker_catches_an_omitted_reverse_source():
    case = J.case("n600_random_k15")
    _fails(case, *J.run(case, "cpu", R=0), match="decidedly farther|id set differs")


def test_checker_catches_an_off_by_one_reverse_offset():
    case = J.case("n600_random_k15")
    _fails(case, *J.run(case, "cpu", off=case.off + 1), match="no candidate|decidedly farther|id set differs")


def test_checker_catches_a_duplicate_id():
    case = J.case("n65_ring_k15")
    keys, ids = J.run(case, "cpu")
    ids = ids.clone()
    ids[7, 3] = ids[7, 2]
    _fails(case, keys, ids, match="twice")


def test_checker_catches_a_tie_given_to_the_higher_id():
    case = J.case("n65_ring_k15")
    keys, ids = J.run(case, "cpu")
    tie = torch.nonzero(keys[:, 1:] == keys[:, :-1])
    assert tie.shape[0] > 0, "the lattice case holds no tie"
    r, c = tie[0].tolist()
    ids = ids.clone()
    ids[r, c], ids[r, c + 1] = ids[r, c + 1].item(), ids[r, c].item()
    _fails(case, keys, ids, match="not ascending")


def test_checker_catches_a_stale_distance():
    """A listed neighbour that kept the distance of the graph it came from (here: 0.1 % off the
    pair's own, the order intact) instead of being re-scored."""
    case = J.case("n600_random_k15")
    keys, ids = J.run(case, "cpu")
    keys = keys.clone()
    keys[11, -1] = keys[11, -1] * 1.001
    _fails(case, keys, ids, match="off its bound")


def test_checker_catches_expanded_form_distances():
    """|x|^2 + |y|^2 - 2 x.y on the near-duplicate rows: D = 2^-20 under norms of 30."""
    A = C.near_duplicates()
    N = A.shape[0]
    case = J.Join("near_duplicates", A, "sqeuclidean", J.start_graph("ring", N, N - 1, 0), 1, 0, 0, 0, False)
    keys, ids = J.run(case, "cpu")
    J.check_join(case, keys, ids)  # the direct form passes
    X = C.dense64(A).float()
    sq = (X * X).sum(1)
    exp = (sq.view(-1, 1) + sq[ids.clamp_min(0)] - 2.0 * torch.einsum("qn,qkn->qk", X, X[ids.clamp_min(0)])).clamp_min(0)
    exp = torch.where(ids >= 0, exp, torch.full_like(exp, float("inf")))
    exp, j = torch.sort(exp, dim=1, stable=True)
    _fails(case, exp, ids.gather(1, j), match="off its bound")
