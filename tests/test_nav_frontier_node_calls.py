"""The other layers of the exploration frontiers (include/tbnav_nav.h G10-G16): the compile-only exploring node, the shim's new members
in the host library, and the new symbols declared in the header and exported by the device library."""
import os

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj")
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")

FIND = b"_ZN7planner9GoalField13findFrontiersERN8bmapping14ParticleFilterEi"     # planner::GoalField::findFrontiers(bmapping::ParticleFilter&, int)
SOLVE_TO = b"_ZN7planner9GoalField16solveToFrontiersEv"
MARK = b"_ZN7planner9GoalField11markVisitedEddd"
CLEAR = b"_ZN7planner9GoalField12clearVisitedEv"
SOLVE_GOALS = b"_ZN7planner9GoalField10solveGoalsE"
SET_COST_FROM = b"_ZN7planner9GoalField11setCostFromERN8bmapping14ParticleFilterEddd"
SLAM = b"_ZN8bmapping14ParticleFilter4SLAM"
APPLY_TO = b"_ZN7planner9GoalField7applyToERN10controller4MPPIEdd"

SYMBOLS = ("tbnav_nav_find_frontiers", "tbnav_nav_profile_find_frontiers", "tbnav_nav_last_frontiers", "tbnav_nav_last_frontier_kernels",
           "tbnav_nav_mark_visited", "tbnav_nav_clear_visited", "tbnav_nav_get_visited", "tbnav_nav_solve_goals", "tbnav_nav_solve_frontiers",
           "tbnav_nav_get_frontier_labels", "tbnav_nav_frontier_list")


def _read(path):
    assert os.path.exists(path), "run __graft_entry__.build()"
    with open(path, "rb") as fh:
        return fh.read()


def test_the_exploring_node_compiles_and_the_host_library_has_the_members():
    node = _read(os.path.join(OBJ, "node_calls_nav_frontier.o"))
    for sym in (SLAM, SET_COST_FROM, FIND, SOLVE_TO, APPLY_TO, MARK, CLEAR, SOLVE_GOALS):
        assert sym in node, sym
    assert b"_ZN7planner9GoalField5solveEdd" not in node          # no waypoint is typed: the goals come from the map
    host = _read(HOST_LIB)
    for sym in (FIND, SOLVE_TO, MARK, CLEAR, SOLVE_GOALS):
        assert sym in host, sym
    older = _read(os.path.join(OBJ, "node_calls_nav_from_filter.o"))
    assert FIND not in older and SOLVE_TO not in older             # the node with a waypoint is as it was


def test_the_symbols_are_declared_and_exported():
    capi = g.load_package().capi
    declared = capi.declared_symbols()
    L = capi.lib()
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name        # capi.py gives each a typed signature
