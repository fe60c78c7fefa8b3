"""Record the GEMM planner's routes (csrc/xg_gemm_route.h; host only, no GPU) into tests/golden/gemm_routes.json:

    python tools/gen_gemm_routes_golden.py [--check]

Compiles tools/gemm_route_dump.cc with g++ and runs it over tests/gemm_shapes.table_inputs().  tests/test_gemm_routes_cpu.py
asserts the table: a change of the routing shows as a diff of this file.  --check compares instead of writing.
File: {"keys": [route members], "routes": {"<input line>": [their values]}}."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "gemm_routes.json")
SRC = os.path.join(ROOT, "tools", "gemm_route_dump.cc")


def build_dump(outdir, extra=()):
    exe = os.path.join(str(outdir), "gemm_route_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, SRC, "-o", exe], check=True)
    return exe


def routes(exe, inputs):
    """[route dict] of the planner for the input dicts, in order"""
    from tests import gemm_shapes as gs
    text = "".join(gs.key(e) + "\n" for e in inputs)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(inputs), (len(out), len(inputs))
    return [json.loads(line) for line in out]


def table(exe):
    from tests import gemm_shapes as gs
    inputs = gs.table_inputs()
    rs = routes(exe, inputs)
    keys = list(rs[0].keys())
    return {"keys": keys, "routes": {gs.key(e): [r[k] for k in keys] for e, r in zip(inputs, rs)}}


def dumps(tab):
    rows = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in tab["routes"].items())
    return '{"keys": %s,\n"routes": {\n%s\n}}\n' % (json.dumps(tab["keys"]), rows)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        tab = table(build_dump(d))
    if "--check" in sys.argv:
        sys.exit(0 if json.load(open(PATH)) == tab else 1)
    with open(PATH, "w") as f:
        f.write(dumps(tab))
    print("%d routes, %d bytes" % (len(tab["routes"]), os.path.getsize(PATH)))
