"""The contract between metmhn_amd/model.py and the modules its definitions live in (results.py, order_host.py,
lattice_host.py), which the other tests and the tools rely on without asserting it: the names metmhn_amd.model offers,
the module-level names tests and tools read or replace there, and that the host definitions are methods reached through
the instance, so that replacing one on an instance is seen by its callers.  No GPU, under a second."""
import numpy as np

import metmhn_amd.lattice_host as lattice_host
import metmhn_amd.model as model_mod
import metmhn_amd.order_host as order_host
import metmhn_amd.results as results
from metmhn_amd.state import MetState
from order_common import host_only, model, paired  # noqa: F401  (host_only is a fixture)

PUBLIC = [
    "GENOTYPE_STRATA", "GenotypeDistribution", "GenotypeSummary", "METASTASIS_STRATA", "MetMHN", "MetState",
    "MetastasisDistribution", "MetastasisSummary", "OrderPosition", "OrderPositions", "OrderPosterior", "OrderPosteriors",
    "OrderPrecedence", "OrderPrecedences", "OrderSample", "OrderSamples", "OrderSnapshot", "OrderSnapshots", "OrderTime",
    "OrderTimes", "PARTNER_STRATA", "PartnerDistribution", "PartnerSummary", "SeedingForecast", "SeedingForecasts",
    "SeedingLandscape", "SimpleNamespace", "State", "annotations", "np", "warnings",
]


def test_public_names_of_the_module():
    assert sorted(name for name in vars(model_mod) if not name.startswith("_")) == sorted(PUBLIC)


def test_names_that_tests_and_tools_read_or_replace():
    for name in ("_ROW_ERRORS", "_subset_sums", "_kronvec"):
        assert hasattr(model_mod, name), name
    assert model_mod._subset_sums is order_host._subset_sums
    homes = (results, order_host, lattice_host)
    for name, value in vars(model_mod).items():                 # one object, whichever module it is imported from
        for home in homes:
            if not name.startswith("__") and getattr(value, "__module__", None) == home.__name__:
                assert getattr(home, name) is value, name


def test_a_method_replaced_on_the_instance_is_seen(host_only):
    n = 5
    mod, plain = model(n, 0), model(n, 0)
    state = MetState.from_seq(paired(n, [0, 1, 3], [1, 2], 1)[:2 * n + 1])
    calls, tables = [], mod._paired_tables

    def counting(st, first_obs):
        calls.append(first_obs)
        return tables(st, first_obs)

    mod._paired_tables = counting
    got = mod.order_posterior(state, "isPaired", "PT")
    assert calls == ["PT"]
    want = plain.order_posterior(state, "isPaired", "PT")
    assert got.log_evidence == want.log_evidence and np.array_equal(got.pre, want.pre)
    assert np.array_equal(got.seed_pos, want.seed_pos)
