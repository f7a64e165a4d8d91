"""host/test/node_calls_device_icp.cpp: turtle_mapping_node.cpp's construction of ScanAlignment and ParticleFilter, compiled
with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP (the define that gives an unchanged node the device ICP).  build() compiles it
(host/Makefile); the object must be there."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_built_with_the_device_icp_define_compiles():
    obj = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj", "node_calls_device_icp.o")
    assert os.path.exists(obj), "run __graft_entry__.build()"
    with open(obj, "rb") as f:
        assert b"useDeviceICP" in f.read()   # the constructor's default argument calls it
