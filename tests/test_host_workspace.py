"""Ownership rules of the C-ABI host code, read off its sources (lmc_atomi_amd/csrc/*.hip, *.h; no GPU, no build).

  * The per-device workspace of the stateless calls (`scratch_here`) is named only where it is declared (lmc_host.h) and in the two files that hold
    stateless extern "C" entry points (lmc_capi.hip, lmc_sapg.hip): no helper takes it on behalf of a sampler handle, which works in its own.
  * lmc_sampler.hip frees nothing itself: what a handle owns goes through an owner (`Owned`, `Workspace`, the accumulators), whose `release()` frees it."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmc_atomi_amd", "csrc")


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) > 20, paths
    return {os.path.basename(p): open(p, encoding="utf-8").read() for p in paths}


def without_release_bodies(text):
    """`text` without the brace-matched body of every function named release."""
    out, pos = [], 0
    for m in re.finditer(r"\brelease\s*\([^)]*\)\s*(const\s*)?\{", text):
        if m.start() < pos:
            continue
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        assert depth == 0, "unbalanced braces after " + m.group(0)
        out.append(text[pos:m.end()])
        pos = i - 1
    out.append(text[pos:])
    return "".join(out)


def test_only_the_stateless_entry_points_name_the_device_scratch():
    users = sorted(name for name, text in sources().items() if re.search(r"\bscratch_here\b", text))
    assert users == ["lmc_capi.hip", "lmc_host.h", "lmc_sapg.hip"], users


def test_the_device_scratch_is_taken_inside_extern_c_only():
    """In the two .hip files every use but the definition stands after the `extern "C" {` that opens the entry points."""
    for name in ("lmc_capi.hip", "lmc_sapg.hip"):
        text = sources()[name]
        entry = text.rindex('extern "C" {')
        for m in re.finditer(r"\bscratch_here\b", text):
            line = text[text.rfind("\n", 0, m.start()) + 1:text.find("\n", m.start())]
            assert m.start() > entry or line.startswith("Workspace& scratch_here() {"), (name, line)


def test_the_sampler_file_frees_nothing_outside_an_owner():
    text = sources()["lmc_sampler.hip"]
    assert "lmc_sampler_destroy" in text and ".release()" in text
    rest = without_release_bodies(text)
    assert "hipFree(" not in rest and "hipHostFree(" not in rest and "hipEventDestroy(" not in rest, \
        [ln for ln in rest.splitlines() if "hipFree(" in ln or "hipHostFree(" in ln or "hipEventDestroy(" in ln]


def test_release_body_stripping_sees_a_free_outside():
    """The helper of the test above on two small texts: a free inside release() goes, one outside stays."""
    inside = "struct A { void release() { if (p) { (void)hipFree(p); } p = nullptr; } };"
    assert "hipFree(" not in without_release_bodies(inside)
    outside = inside + " void f() { hipFree(q); }"
    assert "hipFree(q)" in without_release_bodies(outside)
