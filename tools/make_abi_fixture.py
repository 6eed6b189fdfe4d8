"""Record what the reference headers say about the drop-in boundary in tests/golden/reference_abi.json (run where
the reference tree can be read): the sizes and offsets its types have when compiled with g++, and CoreAPI_Base's
virtual function names in declaration order.  tests/test_abi_layout.py compares include/ and abi.py with the record,
and the record with the reference tree wherever that tree can be read."""
from __future__ import annotations

import json
import pathlib
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import test_abi_layout as t  # noqa: E402

if __name__ == "__main__":
    if not t.REF_READABLE:
        raise SystemExit(f"{t.REF} cannot be read here")
    with tempfile.TemporaryDirectory() as d:
        layout = t.reference_header_layout(pathlib.Path(d))
    rec = {"source": "RenderSystem/core_api_base.h with platform.h, g++ -std=c++17 (x86-64 Linux)",
           "generator": "tools/make_abi_fixture.py", "layout": layout, "vtable": t.reference_vtable_names()}
    t.GOLDEN.write_text(json.dumps(rec, indent=1) + "\n")
    print(f"{t.GOLDEN}: {len(layout)} sizes / offsets, {len(rec['vtable'])} virtual functions")
