"""CPU-only: the library's host-side answers -- workspace sizes, *_supported, layouts, and the status of every rejected or
empty call of tests/abi_rejections.py -- equal, row by row, the answers recorded in tests/golden/abi_rejections.json.  The
JSON was recorded from the library as it was before the C entry points moved out of ctd_api.hip into their kernel
families' files; it pins each status code and the precedence between them, and is not to be regenerated from the code
under test: a new row is recorded from a library built from the commit that defines the contract,
`python -m tests.abi_rejections THAT_LIBRARY > tests/golden/abi_rejections.json`."""
import json
import os

from tests import abi_rejections as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_rejections.json")
CTD_ERR_HIP = 1000


def test_table_is_sound():
    ids = [ar.row_id(f, o) for f, o, _ in ar.ROWS]
    assert len(set(ids)) == len(ids)
    from connecting_the_dots_amd import _lib
    assert set(f for f, _, _ in ar.ROWS) == set(_lib.SIGNATURES) - {"ctd_version", "ctd_status_string"}
    golden = json.load(open(GOLDEN))
    assert [g[0] for g in golden] == ids, "the table and the recorded answers list different rows"
    for (func, _, kind), (row, answer) in zip(ar.ROWS, golden):
        if kind == "query":
            continue
        # a status at or above CTD_ERR_HIP would mean a call that reached the device; only an empty call may answer CTD_OK
        assert 0 <= answer < CTD_ERR_HIP and (answer == 0) == (kind == "empty"), (row, answer)


def test_host_answers_equal_the_recorded_ones():
    from connecting_the_dots_amd import _lib
    golden = json.load(open(GOLDEN))
    got = ar.run(_lib.lib())
    assert len(got) == len(golden)
    wrong = [(g, w) for g, w in zip(got, golden) if g != w]
    assert not wrong, "%d of %d rows differ, first (got, recorded): %s" % (len(wrong), len(got), wrong[:5])
