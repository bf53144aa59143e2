"""CPU: where every generation call ends up -- the engine method and keywords the model classes choose, the loop (host or device),
selection variant, warnings and refusals the engine chooses -- equals, case by case, the table recorded on the commit before the
routing moved into ``emu_amd/genroute.py`` (tests/generation_route_cases.py says how it was recorded)."""
import os

import pytest

from tests import generation_route_cases as gc


@pytest.fixture(scope="module")
def table(golden_dir):
    return gc.load(os.path.join(golden_dir, "generation_routes.json"))


def test_the_table_belongs_to_this_grid_and_reaches_every_branch(table):
    cases = gc.all_cases()
    assert table["cases"] == len(cases) == len(table["index"]) and table["case_ids_sha256"] == gc.digest(cases)
    assert sorted(set(table["index"])) == list(range(len(table["outcomes"])))
    gc.check_coverage(table)


@pytest.mark.parametrize("level", ["model", "engine"])
def test_every_case_ends_where_the_recorded_table_says(table, level):
    cases = gc.all_cases()
    assert len(cases) == len(table["index"])
    n = 0
    for c, i in zip(cases, table["index"]):
        if c["level"] == level:
            assert gc.run_case(c) == table["outcomes"][i], gc.case_id(c)
            n += 1
    assert n > 2000
