"""The host-side plans of pf_unet, pf_ddpm, pf_encoder and pf_decoder are the recorded ones (-m "not gpu"): parameter table in order, packed blob, workspace sizes
and launch counts per batch / precision / n_cond / plan option / telemetry binding, recomputed from the C ABI (tools/plan_fingerprint.py)
and compared with tests/golden/plan_fingerprint.json.  A change that alters a plan on purpose regenerates the file with
`python tools/plan_fingerprint.py --write` and says so."""
import json
import os

import pytest

from polyffusion_amd import _lib
from tools import plan_fingerprint as pfp


@pytest.fixture(scope="module")
def recorded():
    with open(pfp.GOLDEN) as f:
        return json.load(f)


def test_recorded_document_covers_both_builds_and_every_model(recorded):
    assert set(recorded) == {"default", "f16"}
    for doc in recorded.values():
        assert set(doc) == {n for group in (pfp.UNETS, pfp.DDPMS, pfp.ENCODERS, pfp.DECODERS) for n, *_ in group}
    # the figures the file was recorded with: B = 16, split mode, n_cond 1: launches, all prepared, with telemetry bound
    chd = recorded["default"]["sdf_chd8bar"]
    assert (chd["plan"]["split B16 nc1"][2], chd["plan"]["split B16 nc1"][6], chd["plan absmax"]["split B16 nc1"][2]) == (158, 154, 173)
    small = recorded["default"]["ddpm_small"]["plan"]
    assert (small["f32 B16"][1], small["split B16"][1]) == (117, 110)


@pytest.mark.parametrize("variant", ["", "f16"])
def test_plans_equal_the_recorded_fingerprint(recorded, variant):
    if not os.path.exists(_lib.lib_path(variant)):
        from polyffusion_amd.build import build
        build(verbose=False, variant=variant)
    diff = pfp.differences(recorded[pfp.build_key(variant)], pfp.fingerprint(variant))
    assert not diff, "\n".join(diff[:40])
