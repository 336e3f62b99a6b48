"""CAGRA VPQ on the device: ``srml_cagra_search_vpq_f32`` against ``cagra_cases.oracle_search`` over the
integer reconstruction (bit for bit), its keys against fp64 on generic rows (worst error / bound on an
MI355X: 0.023, docs/coverage.md), its limits, and the compressed model end to end on the GPU."""
import pytest

import cagra_vpq_cases as vc
from spark_rapids_ml_nai_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(vc.ORACLE_CASES))
def test_search_matches_oracle_on_integer_codes(name):
    vc.run_oracle_case(name, "cuda:0")


@pytest.mark.parametrize("n,M,offset", vc.ACCURACY_CASES)
def test_keys_within_the_derived_bound(n, M, offset):
    vc.run_accuracy_case(n, M, offset, "cuda:0")


def test_limits_are_refused(monkeypatch):
    vc.run_limit_cases("cuda:0", monkeypatch)


def test_lds_budget_matches_the_kernel_library():
    for args in [(8, 32, 1, 4, 32, 1, 1, 16, 1), (33, 64, 4, 32, 64, 80, 3, 256, 37),
                 (128, 64, 4, 32, 64, 32, 32, 256, 1024), (128, 512, 1, 32, 512, 10, 64, 16, 37),
                 (36, 64, 4, 32, 64, 20, 12, 32, 5), (128, 64, 1, 64, 64, 31, 128, 256, 1)]:
        assert int(ops.native.lib().srml_cagra_vpq_lds_bytes(*args)) == ops.cagra_vpq_lds_bytes(*args), args


@pytest.mark.parametrize("case", [vc.run_model_case, vc.run_exhaustive_model_case], ids=lambda f: f.__name__)
def test_model(case):
    case()
