"""The spill kernels (wdpm_amd/csrc/wdpm_pond_spills.hip) on grounds that put chosen targets into chosen lanes of their waves: the
7 / 8 / 9 boundary of push_group's vote, the live forest voting differently from the forest, more hubs in a wave than tries, failed
votes before and after one that succeeds, a wave whose lane 0 has no target, a ring's mark summed together with seven other
lanes, a hub of hubs whose lanes still share targets after a doubling, N at the wave and block edges, and passes that end in
either buffer (tests/test_pond_spill_scenes.py::test_every_pass_ends_in_either_buffer says which case ends where).  The scenes and
what each must give on the model are those of tests/pond_spill_cases.py, asserted without a device in
tests/test_pond_spill_scenes.py and here again before the device is asked.  Every case holds what tests/test_pond_spills.py
holds: the whole spill table and the counts equal to the model, the invariants on the device's own tables, every older table bit
for bit against a twin context's label_curves(), guard bytes clean.  Integers throughout: no tolerance."""
import pytest

from pond_spill_cases import CASES
from test_pond_spills import check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_scene_on_the_device(hip, name):
    """vote_boundary, live_is_not_forest and cascade run under headroom tolerances of 0 and 0.5 m on one handle"""
    scene, claim, calls = CASES[name]
    dem, water = scene()
    t, s = check(hip, dem, water, claim, calls=calls)
    assert s["ponds"] == len(t) >= 2
