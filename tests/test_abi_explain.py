"""The C-ABI additions of ks_explain: ks_candidate, ks_explanation and the new
symbol against a compiled probe of include/ksched.h (no GPU: loads and layouts
only); the ABI version stays 6 and ks_result / ks_pod / ks_node_score keep
their layouts."""
import ctypes as C
import subprocess
from pathlib import Path

from ksched import _abi

ROOT = Path(__file__).resolve().parent.parent

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "ksched.h"
#define S(t) printf(#t " %zu\n", sizeof(t));
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f));
int main(void) {
  S(ks_candidate) O(ks_candidate, slot) O(ks_candidate, _pad) O(ks_candidate, score)
  S(ks_explanation) O(ks_explanation, num_all_nodes) O(ks_explanation, feasible_nodes) O(ks_explanation, n_candidates)
  O(ks_explanation, top_score_nodes) O(ks_explanation, top_score)
  S(ks_result) S(ks_pod) S(ks_node_score)
  printf("KS_EXPLAIN_MAX_CANDIDATES %d\n", (int)KS_EXPLAIN_MAX_CANDIDATES);
  printf("KSCHED_ABI_VERSION %d\n", (int)KSCHED_ABI_VERSION);
  return 0;
}
"""


def probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in lines if line)}


def test_layouts_match_c(tmp_path):
    got = probe(tmp_path)
    types = {"ks_candidate": _abi.KsCandidate, "ks_explanation": _abi.KsExplanation, "ks_node_score": _abi.KsNodeScore}
    for key, val in got.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(types[t], f).offset == val, key
        elif key in types:
            assert C.sizeof(types[key]) == val, key
    assert got["ks_candidate"] == 64 and got["ks_explanation"] == 24 and got["ks_node_score"] == 56
    assert got["ks_candidate.score"] == 8 and got["ks_explanation.top_score"] == 16
    assert got["KS_EXPLAIN_MAX_CANDIDATES"] == 128 == _abi.EXPLAIN_MAX_CANDIDATES
    assert got["ks_result"] == 64 and got["ks_pod"] == 184 and got["KSCHED_ABI_VERSION"] == 6


def test_new_symbol_exported():
    lib = _abi.ksched_lib()
    assert "ks_explain" in _abi.KSCHED_SYMBOLS and hasattr(lib, "ks_explain")
    assert lib.ks_abi_version() == 6
    # a null context is refused before anything else
    assert lib.ks_explain(None, None, 1, None, None) == _abi.KS_ERR_INVALID
    from ksched import Explanation, NodePluginScores, Scheduler
    assert hasattr(Scheduler, "explain")
    assert Explanation.__dataclass_fields__.keys() == {
        "num_all_nodes", "feasible_nodes", "top_score", "top_score_nodes", "candidates"}
    assert {"name", "scores", "total_score", "slot", "raw"} <= NodePluginScores.__dataclass_fields__.keys()
    # the three-argument form the schedule_pod hook uses stays
    assert NodePluginScores("n", [], 7).total_score == 7
