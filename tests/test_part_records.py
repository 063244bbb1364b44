"""The packed partition records, byte for byte (tests/golden/part_records.json).

tests/golden/make_part_records.py holds the cases: synthetic colour and AOV states split into parts, packed by the
numpy restatement and merged by the C host twins.  The committed file holds the SHA-256 of every record and merged
array and the host twins' refusals; this test recomputes them on the current tree.  CPU only."""
import json

import pytest

from tests.golden import make_part_records as M


@pytest.fixture(scope="module")
def golden():
    with open(M.PATH) as f:
        return json.load(f)


def test_every_case_is_covered(golden):
    keys = set(golden["digests"])
    for tile in ("8x8", "5x3"):
        for flags in range(8):
            for n in (1, 2, 3, 7, 30 if tile == "8x8" else 87):
                assert f"colour tile {tile} flags {flags} parts {n}" in keys
    for channels in range(1, 8):
        for n in (1, 2, 3, 30):
            assert f"aov channels {channels} parts {n}" in keys
    assert len(keys) == 2 * 8 * 5 + 7 * 4
    assert all(len(v) == 64 for v in golden["digests"].values())


def test_records_and_merges_keep_their_bytes(golden):
    got = M.digests()
    assert set(got) == set(golden["digests"])
    differ = [k for k in got if got[k] != golden["digests"][k]]
    assert not differ, differ


def test_adaptive_cases_hold_stopped_parts():
    s = M.colour_state((8, 8), 7)
    assert (s.tile_stop != 0).any() and (s.tile_stop == 0).any()
    parts = s.split(3)
    assert (parts[1].tile_stop != 0).all() and parts[1].samples < M.SAMPLES  # every tile of part 1 has stopped
    assert any(p.slots == 0 for p in s.split(30))  # parts without tiles


def test_host_twins_refuse_as_before(golden):
    got = M.refusals()
    assert got == golden["refusals"]
    for kind in ("colour", "aov"):
        for reason, (rc, message) in got[kind].items():
            assert rc == 1 and reason.split(" ")[0] in message, (kind, reason, message)
