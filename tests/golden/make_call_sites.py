#!/usr/bin/env python3
"""Which attributes of its detection / preprocessing / stats modules the reference's callers use, and the signatures of
the functions chromosight_amd.integration rebinds: data for tests/test_integration_recipe.py (needs a checkout of the
reference; the tests themselves read only the JSON files written here).

    python tests/golden/make_call_sites.py <reference checkout>

Parses chromosight/cli/chromosight.py and chromosight/utils/contacts_map.py with `ast`: `import ... as <alias>` of the
three modules, then every `<alias>.<attr>` and every `from <module> import <name>`; writes reference_call_sites.json
{module: {attr: [file:line, ...]}}.  Imports the reference's three modules and writes reference_signatures.json
{module: {function: [{"name": parameter, "default": value} ...]}} for every function of integration.REBIND: "default" is
absent for a parameter without one, and a callable default is recorded as {"callable": true}."""
import ast
import importlib
import inspect
import json
import pathlib
import sys

HERE = pathlib.Path(__file__).resolve().parent
MODULES = {"chromosight.utils.detection": "detection", "chromosight.utils.preprocessing": "preprocessing",
           "chromosight.utils.stats": "stats"}


def call_sites(ref):
    out = {m: {} for m in MODULES.values()}
    for path in [ref / "chromosight" / "cli" / "chromosight.py", ref / "chromosight" / "utils" / "contacts_map.py"]:
        tree = ast.parse(path.read_text())
        alias = {}
        rel = f"{path.parent.name}/{path.name}"
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                for a in node.names:
                    if a.name in MODULES:
                        alias[a.asname or a.name] = MODULES[a.name]
            elif isinstance(node, ast.ImportFrom) and node.module in MODULES:
                for a in node.names:
                    out[MODULES[node.module]].setdefault(a.name, []).append(f"{rel}:{node.lineno}")
            elif isinstance(node, ast.ImportFrom) and node.level == 1 and node.module is None and path.parent.name == "utils":
                for a in node.names:                     # from . import preprocessing as preproc
                    full = f"chromosight.utils.{a.name}"
                    if full in MODULES:
                        alias[a.asname or a.name] = MODULES[full]
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in alias:
                out[alias[node.value.id]].setdefault(node.attr, []).append(f"{rel}:{node.lineno}")
    return {m: {k: sorted(set(v)) for k, v in sorted(out[m].items())} for m in out}


def signatures(ref):
    sys.path.insert(0, str(HERE.parents[1]))
    from chromosight_amd import integration
    sys.path.insert(0, str(ref))
    out = {}
    for module, names in integration.REBIND.items():
        mod = importlib.import_module(f"chromosight.utils.{module}")
        out[module] = {}
        for name in names:
            params = []
            for p, v in inspect.signature(getattr(mod, name)).parameters.items():
                entry = {"name": p}
                if v.default is not inspect.Parameter.empty:
                    entry["default"] = {"callable": True} if callable(v.default) else v.default
                params.append(entry)
            out[module][name] = params
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = pathlib.Path(sys.argv[1]).resolve()
    sites = call_sites(ref)
    (HERE / "reference_call_sites.json").write_text(json.dumps(sites, indent=1) + "\n")
    (HERE / "reference_signatures.json").write_text(json.dumps(signatures(ref), indent=1) + "\n")
    print(json.dumps(sites, indent=1))


if __name__ == "__main__":
    main()
