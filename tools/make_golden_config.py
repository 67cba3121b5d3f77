#!/usr/bin/env python3
"""Golden field list of the reference's ``VapConfig`` (rvap/vap_main/vap_main.py:35-66): the names of its annotated fields, in
declaration order, read with ``ast`` (the module is not imported).  Only the names are stored.
Output: tests/golden/vapconfig_fields.json (checked by tests/test_level1_construction.py).

Usage:  python tools/make_golden_config.py <reference checkout>
"""
import ast
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

txt = open(os.path.join(sys.argv[1], "rvap", "vap_main", "vap_main.py")).read()
cls = next(n for n in ast.parse(txt).body if isinstance(n, ast.ClassDef) and n.name == "VapConfig")
fields = [n.target.id for n in cls.body if isinstance(n, ast.AnnAssign)]
with open(os.path.join(REPO, "tests", "golden", "vapconfig_fields.json"), "w") as f:
    json.dump(fields, f)
    f.write("\n")
print(fields)
