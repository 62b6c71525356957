"""The drop-in's mate-pair path support (include/mg_api.hpp):
OverlapGraph::findSupportByMatepairsAndMerge with its counter accessors, driven
through the CLI (mg_overlap -support), a C++ caller of mg_api.hpp that
prints the reference's summary lines and writes <prefix>.support.unitig.
Against the reference's own counts and .unitig bytes after its merge
(tests/golden/make_paths_golden.py): after the build path (new OverlapGraph(ht)
-> sortEdges -> calculateMeanAndSdOfInsertSize) on the four paired fixtures and
after the resume path on the hand cases, once with the search on the device
(MG_DEVICE_PATHS=1) and once by the host mirror (MG_DEVICE_PATHS=0)."""
import pytest

import paths_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", ["1", "0"])
@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES)
def test_build_path(name, device, tmp_path):
    g = R.golden(name)
    lines, unitig = R.run_cli_support(g, tmp_path, resume=False, env={"MG_DEVICE_PATHS": device})
    assert lines == R.summary_lines(g)
    assert unitig == g.unitig_after


@pytest.mark.parametrize("name", R.hand_case_names())
def test_resume_path_on_the_device(name, tmp_path):
    g = R.hand_cases()[name]
    lines, unitig = R.run_cli_support(g, tmp_path, resume=True, env={"MG_DEVICE_PATHS": "1"})
    assert lines == R.summary_lines(g)
    assert unitig == g.unitig_after
