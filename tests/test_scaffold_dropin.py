"""The drop-in's scaffolder (include/mg_api.hpp): OverlapGraph::scaffolder()
driven through the CLI (mg_overlap -scaffold), a C++ caller of mg_api.hpp that
runs calculateMeanAndSdOfInsertSize and one scaffolder(), whose lines go to
stdout, and writes <prefix>.scaffold.unitig.  Against the reference's own lines,
character for character, and its .unitig bytes after the merge
(tests/golden/make_scaffold_golden.py): after the build path on the paired
fixtures and after the resume path on the hand cases, with the scoring on the
device (MG_DEVICE_SCAFFOLD=1) and by the host mirror (MG_DEVICE_SCAFFOLD=0; on
the resume path that run needs no device)."""
import pytest

import scaffold_ref as R


@pytest.mark.gpu
@pytest.mark.parametrize("device", ["1", "0"])
@pytest.mark.parametrize("name", R.GOLDEN_FIXTURES)
def test_build_path(name, device, tmp_path):
    g = R.golden(name)
    lines, unitig = R.run_cli_scaffold(g, tmp_path, resume=False, env={"MG_DEVICE_SCAFFOLD": device})
    assert lines == g.raw_lines
    assert lines.count("\n") == g.merged
    if g.unitig_after is not None:
        assert unitig == g.unitig_after


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.hand_case_names())
def test_resume_path_on_the_device(name, tmp_path):
    g = R.hand_cases()[name]
    lines, unitig = R.run_cli_scaffold(g, tmp_path, resume=True, env={"MG_DEVICE_SCAFFOLD": "1"})
    assert lines == g.raw_lines and lines.count("\n") == g.merged
    assert unitig == g.unitig_after


@pytest.mark.parametrize("name", R.hand_case_names())
def test_resume_path_by_the_mirror(name, tmp_path):
    g = R.hand_cases()[name]
    env = {"MG_DEVICE_SCAFFOLD": "0", "MG_DEVICE_PLACES": "0"}
    lines, unitig = R.run_cli_scaffold(g, tmp_path, resume=True, env=env)
    assert lines == g.raw_lines and lines.count("\n") == g.merged
    assert unitig == g.unitig_after
