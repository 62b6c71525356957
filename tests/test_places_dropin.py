"""The drop-in's insert sizes and coverage (include/mg_api.hpp):
OverlapGraph::calculateMeanAndSdOfInsertSize / getMean / getSD, Edge::
coverageDepth and Edge::SD from calculateCoverageOfAllEdges (one device call)
and from getBaseByBaseCoverage(Edge*) (the host mirror), against the
reference's own values (tests/golden/make_places_golden.py): after the build
path (new OverlapGraph(ht) -> sortEdges, a context of the drop-in's own) on the
paired-end fixtures, after the resume path on the hand cases, with the device
and with MG_DEVICE_PLACES=0.  Driven through the CLI (mg_overlap -insert), a
C++ caller of mg_api.hpp, which prints the reference's stdout lines."""
import pytest

import places_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", ["1", "0"])
@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES)
def test_build_path(name, device, tmp_path):
    g = R.golden(name)
    lines, rows = R.run_cli_insert(g, tmp_path, resume=False, env={"MG_DEVICE_PLACES": device})
    assert lines == g.stdout
    assert [ln for ln in lines if ln.startswith("Mean")] == ["Mean set to: %d" % d[0] for d in g.datasets if d[2]]
    assert rows == R.golden_coverage_rows(g)


@pytest.mark.parametrize("name", R.HAND_CASES)
def test_resume_path_on_the_device(name, tmp_path):
    g = R.hand_cases()[name]
    lines, rows = R.run_cli_insert(g, tmp_path, resume=True, env={"MG_DEVICE_PLACES": "1"})
    assert lines == g.stdout
    assert rows == R.golden_coverage_rows(g)
