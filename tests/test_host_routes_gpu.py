"""GPU: the host path reaches the same native calls, in the same order, with the same bits as before the route decision was gathered
into losses._route.  tests/golden/host_routes.json is the output of tools/record_host_routes.py at the commit before that refactor; the
lattice is replayed once here and every case is held to its record: the ordered names of the work-enqueuing callables, the grad_fn class,
dtype and shape of the result, the warn_once keys, and -- for every case that does not take the torch-op composition -- the SHA-256 of
the loss and of each gradient.  (wasserstein_1d no longer wraps a call without a gradient in _RowLoss.apply; such a result had no grad_fn
before either, so no case of the record is exempted from equality.)"""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT
from gpu_util import device, native

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "host_routes.json")) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def replay():
    native()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_host_routes
    finally:
        sys.path.pop(0)
    return record_host_routes.record(device())


def test_the_lattice_is_the_recorded_one(replay):
    assert sorted(replay) == sorted(RECORD)
    composition = [k for k, v in RECORD.items() if any(n in ("module_forward", "transport_rows") for n in v["names"])]
    hashed = [k for k, v in RECORD.items() if "loss_sha256" in v]
    assert not any("error" in v for v in RECORD.values()) and not any("error" in v for v in replay.values())
    assert len(hashed) + len(composition) == len(RECORD)   # only the composition skips the hashes
    assert len(hashed) > 200 and not set(hashed) & set(composition)


@pytest.mark.parametrize("case", sorted(RECORD))
def test_case_equals_its_record(replay, case):
    assert replay[case] == RECORD[case]
