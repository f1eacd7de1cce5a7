"""The host layer of libicamd.so (csrc/capi*.hip) without a GPU: every size / support query gives the recorded answer, and every
launching entry refuses what it refused, with the same return code.  The answers (tests/golden/capi_answers.json) were recorded
from the library of the commit BEFORE the C-ABI layer was split into units, by tests/golden/make_capi_answers.py, whose docstring
says what a record holds and why no call here can launch anything."""
import importlib.util
import json
import os

import pytest

from imageclassification_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_capi_answers", os.path.join(GOLDEN, "make_capi_answers.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(os.path.join(GOLDEN, "capi_answers.json")) as f:
    FIXTURE = json.load(f)


def test_fixture_covers_every_entry():
    """30 queries, each nonzero somewhere; every other entry that launches has its refusal; the cases are the generator's."""
    queries, launching = G.query_names(), G.launching_names()
    assert len(queries) == 30 and "icamd_colsum_rows" not in queries and "icamd_colsum_rows" in launching
    assert set(queries) | set(launching) | set(G.NOT_LAUNCHING) == set(hip._SIGNATURES)
    assert list(FIXTURE["queries"]) == queries and list(FIXTURE["refusals"]) == launching
    for name, rows in FIXTURE["queries"].items():
        assert [a for a, _ in rows] == [list(a) for a in G.QUERY_ARGS[name]], name
        assert any(v != 0 for _, v in rows), name
    assert all(rc != 0 for rc in FIXTURE["refusals"].values())
    assert [[n, a] for n, a, _ in FIXTURE["ordered"]] == G.ORDERED_REFUSALS
    assert {rc for _, _, rc in FIXTURE["ordered"]} == {1, 2, 3}       # BAD_ARG, UNSUPPORTED and WORKSPACE all occur, LAUNCH never


@pytest.mark.parametrize("name", list(FIXTURE["queries"]))
def test_query_answers_are_the_recorded_ones(name):
    lib = hip.load()
    assert [[a, G.ask(lib, name, a)] for a, _ in FIXTURE["queries"][name]] == FIXTURE["queries"][name]


def test_all_zero_calls_are_refused_with_the_recorded_codes():
    lib = hip.load()
    assert {n: G.refuse(lib, n) for n in FIXTURE["refusals"]} == FIXTURE["refusals"]


def test_ordered_refusals_give_the_recorded_codes():
    lib = hip.load()
    assert [[n, a, G.ask(lib, n, a)] for n, a, _ in FIXTURE["ordered"]] == FIXTURE["ordered"]
