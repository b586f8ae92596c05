"""the function-level rebinding recipe (chromosight_amd.integration) against the attributes the
reference's callers actually use (tests/golden/reference_call_sites.json, parsed from cli/chromosight.py and
utils/contacts_map.py by tests/golden/make_call_sites.py) and the signatures of the reference's functions it rebinds
(tests/golden/reference_signatures.json, written by the same script).  CPU only."""
import importlib
import inspect
import json
import pathlib
import types

from chromosight_amd import integration

HERE = pathlib.Path(__file__).resolve().parent
SITES = json.loads((HERE / "golden" / "reference_call_sites.json").read_text())
SIGNATURES = json.loads((HERE / "golden" / "reference_signatures.json").read_text())


def test_every_attribute_the_callers_use_is_rebound_or_kept():
    for module, attrs in SITES.items():
        for name, where in attrs.items():
            assert name in integration.REBIND[module] or name in integration.KEEP[module], (module, name, where)
    # the call sites the boundary is about
    assert "pattern_detector" in SITES["detection"] and "remove_neighbours" in SITES["detection"]
    assert {"detrend", "diag_trim", "valid_to_missing"} <= set(SITES["preprocessing"])
    # what a module swap would have broken: used by the callers, deliberately not in this package
    assert {"get_detectable_bins", "subsample_contacts"} <= set(SITES["preprocessing"])
    assert {"get_detectable_bins", "subsample_contacts"} <= set(integration.KEEP["preprocessing"])


def test_rebound_names_exist_here_and_kept_names_do_not_shadow():
    for module, names in integration.REBIND.items():
        ours = importlib.import_module(f"chromosight_amd.utils.{module}")
        for name in names:
            assert callable(getattr(ours, name, None)), (module, name)
        assert not set(names) & set(integration.KEEP[module])


def test_rebind_and_restore_on_stand_in_modules():
    mods = {k: types.SimpleNamespace(**{n: (lambda *a, _n=n: _n) for n in integration.REBIND[k] + integration.KEEP[k]})
            for k in integration.REBIND}
    kept = {k: {n: getattr(mods[k], n) for n in integration.KEEP[k]} for k in mods}
    prev = integration.rebind(**mods)
    import chromosight_amd.utils.detection as cud
    import chromosight_amd.utils.preprocessing as cup
    assert mods["detection"].pattern_detector is cud.pattern_detector
    assert mods["preprocessing"].detrend is cup.detrend
    for k in mods:
        for n in integration.KEEP[k]:
            assert getattr(mods[k], n) is kept[k][n]            # untouched
    integration.restore(prev, **mods)
    assert mods["detection"].pattern_detector() == "pattern_detector"


def test_signatures_match_the_reference():
    """Same parameter names, order and defaults as the reference for every rebound function (the reference's signatures
    as tests/golden/make_call_sites.py recorded them)."""
    for module, names in integration.REBIND.items():
        assert sorted(SIGNATURES[module]) == sorted(names), module
        ours = importlib.import_module(f"chromosight_amd.utils.{module}")
        for name in names:
            a = SIGNATURES[module][name]
            b = inspect.signature(getattr(ours, name)).parameters
            assert [p["name"] for p in a] == list(b), (module, name, [p["name"] for p in a], list(b))
            for p in a:
                db = b[p["name"]].default
                assert ("default" in p) == (db is not inspect.Parameter.empty), (module, name, p["name"])
                if "default" in p and p["default"] != {"callable": True}:
                    assert p["default"] == db, (module, name, p["name"], p["default"], db)
