"""Which engine a call of the FIR family takes (csrc/fir_plan.h), on the CPU: host/fir_plan_test.cc checks the properties
every route must have over a sweep of kinds, decimations, tap counts, capability sets, modes and call facts, and the
shapes whose tests or documents name their engine, under the address and undefined-behaviour sanitizers, as a program
of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")


def test_routes_hold_their_properties_and_named_shapes_their_engine():
    r = subprocess.run(["make", "-C", HOST, "fir_plan_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "fir_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
