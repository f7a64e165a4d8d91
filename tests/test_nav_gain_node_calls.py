"""The other layers of the frontiers ranked by information gain (include/tbnav_nav.h G17-G20): the compile-only ranking node, the shim's
new members in the host library, and the new symbols declared in the header and exported by the device library."""
import os

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj")
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")

FIND_GAIN = b"_ZN7planner9GoalField17findFrontiersGainERN8bmapping14ParticleFilterEdi"     # planner::GoalField::findFrontiersGain(bmapping::ParticleFilter&, double, int)
SOLVE_RANKED = b"_ZN7planner9GoalField22solveToFrontiersRankedEi"
LAST_GAIN = b"_ZNK7planner9GoalField8lastGainEv"
GAIN = b"_ZN7planner9GoalField12frontierGainEv"
GAIN_LIST = b"_ZN7planner9GoalField16frontierGainListEv"
GAIN_KERNELS = b"_ZNK7planner9GoalField15lastGainKernelsB5cxx11Ev"
PROFILE = b"_ZN7planner9GoalField24profileFindFrontiersGainERN8bmapping14ParticleFilterEdi"
FIND = b"_ZN7planner9GoalField13findFrontiersERN8bmapping14ParticleFilterEi"
SOLVE_TO = b"_ZN7planner9GoalField16solveToFrontiersEv"
SET_COST_FROM = b"_ZN7planner9GoalField11setCostFromERN8bmapping14ParticleFilterEddd"
APPLY_TO = b"_ZN7planner9GoalField7applyToERN10controller4MPPIEdd"
MARK = b"_ZN7planner9GoalField11markVisitedEddd"

SYMBOLS = ("tbnav_nav_gain_rays", "tbnav_nav_find_frontiers_gain", "tbnav_nav_profile_find_frontiers_gain", "tbnav_nav_last_gain",
           "tbnav_nav_last_gain_kernels", "tbnav_nav_get_frontier_gain", "tbnav_nav_frontier_gain_list", "tbnav_nav_solve_frontiers_ranked")


def _read(path):
    assert os.path.exists(path), "run __graft_entry__.build()"
    with open(path, "rb") as fh:
        return fh.read()


def test_the_ranking_node_compiles_and_the_host_library_has_the_members():
    node = _read(os.path.join(OBJ, "node_calls_nav_gain.o"))
    for sym in (SET_COST_FROM, FIND_GAIN, LAST_GAIN, SOLVE_RANKED, APPLY_TO, MARK, GAIN, GAIN_LIST, GAIN_KERNELS, PROFILE):
        assert sym in node, sym
    assert FIND not in node and SOLVE_TO not in node               # the ranked calls stand in place of the plain ones
    host = _read(HOST_LIB)
    for sym in (FIND_GAIN, LAST_GAIN, SOLVE_RANKED, GAIN, GAIN_LIST, GAIN_KERNELS, PROFILE):
        assert sym in host, sym
    older = _read(os.path.join(OBJ, "node_calls_nav_frontier.o"))
    assert FIND_GAIN not in older and SOLVE_RANKED not in older      # the node that drives to the nearest seed is as it was


def test_the_symbols_are_declared_and_exported():
    capi = g.load_package().capi
    declared = capi.declared_symbols()
    L = capi.lib()
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name        # capi.py gives each a typed signature


def test_the_python_mirror_has_the_methods():
    g.load_package()
    from rtn_amd import nav
    for name in ("findFrontiersGain", "lastGain", "frontierGain", "frontierGainList", "solveFrontiersRanked", "lastGainKernels", "profileFindFrontiersGain"):
        assert callable(getattr(nav.GoalField, name)), name
    assert callable(nav.gain_rays)
