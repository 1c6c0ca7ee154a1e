"""records the two structures tests/test_accel_check.py mutates (needs the GPU):   python tests/golden/build_closure/make_fixtures.py [output directory]
   cornell.npz    everything rtgo_set_scene builds for the cornell scene (own boxes), with the scene's types, matrices and materials
   sphere300.npz  what rtgo_whitted_set_mesh builds for a 300-triangle sphere, with the surface-area records ("sah/") and with
                  RTGO_WHITTED_NO_SAH ("morton/"), and the mesh"""
import os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import accel_check as A
from raytracingo_amd import capi, scene as hscene
OUT = sys.argv[1] if len(sys.argv) > 1 else HERE   # (where to write)

t = hscene.tables("cornell", 64, 64)
ctx = capi.Context(0)
ctx.set_scene(t["type"], t["M"], t["mat"], None)
A.record(os.path.join(OUT, "cornell.npz"), ctx.read_build(False), types=np.asarray(t["type"], np.int32), M=np.asarray(t["M"], np.float32),
         mat=np.asarray(t["mat"], np.float32))
ctx.close()

mesh = A.sphere300()
build = {}
for key, no_sah in (("sah/", False), ("morton/", True)):
    os.environ.pop("RTGO_WHITTED_NO_SAH", None)
    if no_sah:
        os.environ["RTGO_WHITTED_NO_SAH"] = "1"
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], None, mesh["materials"])
    build.update({key + k: v for k, v in ctx.read_build(True).items()})
    ctx.close()
A.record(os.path.join(OUT, "sphere300.npz"), build, positions=mesh["positions"], indices=mesh["indices"])
for f in ("cornell.npz", "sphere300.npz"):
    print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")
