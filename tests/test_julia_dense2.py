"""The Julia binding names BASELINE config 5's objective (SMM_OBJ_DENSE2) as the C header and the Python layer do, and the glue maps
opts["hip_objective"] = :dense2 to it.  No julia binary in the image: checked on the text, as test_julia_layer.py does."""
import os
import re

from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = os.path.join(ROOT, "julia", "SMMHip.jl")
GLUE = os.path.join(ROOT, "julia", "SMMHipBackend.jl")


def test_the_binding_defines_obj_dense2_as_the_header_does():
    src = open(RAW).read()
    m = re.search(r"^const OBJ_DENSE2 = Cint\((\d+)\)", src, re.M)
    assert m, "SMMHip.jl: no OBJ_DENSE2"
    assert int(m.group(1)) == A.SMM_OBJ_DENSE2 == 5
    hdr = open(os.path.join(ROOT, "include", "smmhip.h")).read()
    assert re.search(r"SMM_OBJ_DENSE2 = %d\b" % A.SMM_OBJ_DENSE2, hdr)


def test_the_glue_maps_dense2_to_it():
    src = open(GLUE).read()
    assert re.search(r"o == :dense2 && return SMMHip\.OBJ_DENSE2\b", src)
    assert re.search(r"o == :dense && return SMMHip\.OBJ_DENSE\b", src)   # (v1 unchanged)
