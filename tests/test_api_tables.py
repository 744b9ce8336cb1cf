"""The tables of radiosaber_amd/api.py (not gpu): one prototype per function of the header, one row per form of a group call."""
import itertools
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

KEYWORDS = ("group", "resident", "queued", "counted", "flows", "run")
# the keyword sets that select a kernel and the rs_jit_cache_* flag bits of each, as literals; every other set is refused
VALID = {
    frozenset(): 0,
    frozenset({"group"}): 8,
    frozenset({"group", "resident"}): 24,
    frozenset({"group", "queued"}): 40,
    frozenset({"group", "counted"}): 104,
    frozenset({"group", "queued", "counted"}): 104,
    frozenset({"group", "flows"}): 136,
    frozenset({"group", "resident", "run"}): 280,
}
FORM_NAMES = {
    "": ("rs_group_specialize", "rs_group_jit_status", "rs_jit_selfcheck_group"),
    "resident": ("rs_group_specialize_resident", "rs_group_resident_jit_status", "rs_jit_selfcheck_group_resident"),
    "queued": ("rs_group_specialize_queued", "rs_group_queued_jit_status", "rs_jit_selfcheck_group_queued"),
    "counted": ("rs_group_specialize_counted", "rs_group_counted_jit_status", "rs_jit_selfcheck_group_counted"),
    "flows": ("rs_group_specialize_flows", "rs_group_flows_jit_status", "rs_jit_selfcheck_group_flows"),
    "run": ("rs_group_specialize_run", "rs_group_run_jit_status", "rs_jit_selfcheck_group_run"),
}


def _header_functions(ordered=False):
    txt = (ROOT / "include" / "radiosaber_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    if ordered:  # by first declaration; the RS_*_CREATE macros name functions out of turn
        txt = "\n".join(line for line in txt.splitlines() if not line.lstrip().startswith("#define"))
        return list(dict.fromkeys(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", txt)))
    return sorted(set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", txt)))


def test_one_prototype_per_function_of_the_header():
    from radiosaber_amd import api
    declared = _header_functions()
    assert declared, "no prototypes found"
    assert sorted(api.PROTOTYPES) == declared
    assert list(api.PROTOTYPES) == _header_functions(ordered=True), "not in the header's order"
    for name, proto in api.PROTOTYPES.items():
        assert len(proto) == 2 and isinstance(proto[1], list), f"{name} has no argtypes"
    assert api.ABI_SYMBOLS == list(api.PROTOTYPES)


def test_lib_applies_every_prototype(rs):
    from radiosaber_amd import api
    L = rs.lib()
    for name, (restype, argtypes) in api.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_jit_flags_over_all_keyword_sets():
    from radiosaber_amd import api
    returned = 0
    for bits in itertools.product((False, True), repeat=len(KEYWORDS)):
        kw = dict(zip(KEYWORDS, bits))
        on = frozenset(k for k in KEYWORDS if kw[k])
        for lean, streamed in itertools.product((False, True), repeat=2):
            if on in VALID:
                assert api._jit_flags(lean, streamed, **kw) == VALID[on] | (4 if lean else 0) | (2 if streamed else 0), (on, lean, streamed)
            else:
                with pytest.raises(ValueError) as e:
                    api._jit_flags(lean, streamed, **kw)
                assert any(f"{k}=True" in str(e.value) for k in on), (on, str(e.value))  # (the refusal names a keyword that was given)
        returned += on in VALID
    assert returned == 8 and len(VALID) == 8


def test_the_forms_are_the_six_rows_in_order():
    from radiosaber_amd import api
    assert [f.key for f in api.GROUP_FORMS] == list(FORM_NAMES)
    assert [f.flags for f in api.GROUP_FORMS] == [8, 24, 40, 104, 136, 280]
    for f in api.GROUP_FORMS:
        assert (f.specialize, f.jit_status, f.selfcheck) == FORM_NAMES[f.key]


def test_form_names_are_in_the_library_and_the_scheduler(rs):
    from radiosaber_amd import api
    L = rs.lib()
    for f in api.GROUP_FORMS:
        for name in (f.specialize, f.jit_status, f.selfcheck):
            assert hasattr(L, name) and name in api.PROTOTYPES, name
    for key in FORM_NAMES:
        for method in ("specialize" + ("_" + key if key else ""), (key + "_" if key else "") + "jit_status"):
            assert callable(getattr(rs.GroupScheduler, method)), method
