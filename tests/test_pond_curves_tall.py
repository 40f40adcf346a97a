"""The pond stage curves past the strip gate (include/wdpm_pond_curves.h): 300 000 x 3 with WDPM_PONDS_ROWS_PER_WAVE unset, so that
the raster holds more than 32 768 segments and the library itself cuts strips of several rows: beds and stage sums carried down the
rows of a strip as the library chooses them.  One call, held against the numpy model (tests/pond_curves_model.py)."""
import numpy as np
import pytest

from helpers import pad
from test_group_pond_outlets_tall import TABLE_WAVES, noise_scene
from test_pond_curves import MISS, WET, hold_against_model

pytestmark = pytest.mark.gpu


def test_300000_rows_with_the_library_s_own_strips(hip, monkeypatch):
    from wdpm_amd.ponds import Ponds
    monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    R, Cc = 300000, 3
    dem, water = noise_scene(R, Cc)
    bd, bw = pad(dem, water, MISS)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            n = p.label_curves(WET)
            s = p.stats()
            assert s["segments"] > TABLE_WAVES and s["rows_per_wave"] == -(-s["segments"] // TABLE_WAVES) > 1, s
            table, stats, _ = hold_against_model(bd, MISS, bw, WET, p, n)
            assert len(table) > 10000 and stats["stage_cells"] > len(table) and stats["no_curve"] < len(table), stats
            assert (np.diff(table["cells"], axis=1) > 0).any() and p.guard_bad() == 0
