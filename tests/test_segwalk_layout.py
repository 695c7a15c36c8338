"""The segmented walk's entry table and workspace layout, on the CPU: tests/host_cpp/test_segwalk_layout.cpp calls the
library's seg_entries, segwalk_carve and streams_carve (x3_internal.h) over entry tables of 1 to 1 000 entries -- lengths
around the span size, empty tables, overlapping and repeated offsets, the bound on the span count -- and checks the span
counts, the refusals and the carved pieces (disjoint, aligned, long enough, inside the returned size, the entry table in one
piece as its upload needs it).  The same driver calls windows_carve and levels_carve over window and range counts, frame
counts and block lengths around the rounding of 256 bytes, the scratch cap and the grid of four waves, and compares every
piece's offset and the total with the chains of rounded offsets the launches used to write out; and events_carve,
range_levels_carve (with range_levels_pairs at both arms of its min) and quantiles_carve over row counts around the rounding
and the tile edges, 0, 1 and 1 000 entries, 1 and 8 quantiles, against the chains their first carve gave.  Built by tests/test_routes.py's build_driver: the library's translation units compiled, the
driver host code only, no context."""
import os
import subprocess

import pytest

import test_routes as R

DRIVER = os.path.join(R.ROOT, "tests", "host_cpp", "test_segwalk_layout.cpp")


@pytest.mark.skipif(not os.path.exists(R.HIPCC), reason="hipcc not found")
def test_entry_table_and_workspace_layout():
    exe = R.build_driver(DRIVER, "test_segwalk_layout")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok tables="), (r.stdout[-4000:], r.stderr[-2000:])
    counts = dict(kv.split("=") for kv in r.stdout.split()[1:])
    assert int(counts["tables"]) >= 240 and int(counts["carves"]) >= 240, counts
    # 7 counts x 5 frame counts x 5 block lengths x (windows, ranges); 5 x 5 x 3 row counts x 3 entry counts
    assert int(counts["windows"]) >= 350 and int(counts["levels"]) >= 225, counts
    # 17 row counts x 3 entry counts (x 2 quantile counts); 6 range counts x 5 frame counts x 3 x 3 x 2
    assert int(counts["events"]) >= 51 and int(counts["quantiles"]) >= 102 and int(counts["range_levels"]) >= 540, counts
