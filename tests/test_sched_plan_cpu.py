"""The index schedules of pfb_arb_resampler and fractional_interpolator (csrc/sched_plan.h) on the CPU:
host/sched_plan_test.cc runs every closed form against the walk of the reference's float arithmetic, under the address
and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")


def test_closed_forms_equal_the_walks():
    r = subprocess.run(["make", "-C", HOST, "sched_plan_test"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([os.path.join(HOST, "sched_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
