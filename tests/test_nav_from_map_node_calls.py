"""The other layers of the cost grid from the filter's map (include/tbnav_nav.h G7-G9): the compile-only node file that owns filter,
planner and controller, the shims' new methods in the host library, and the course of the behaviour test on the CPU."""
import os

import numpy as np

import nav_from_map_cases as fc
import nav_from_map_restatement as fr
import nav_restatement as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj")
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")

SET_COST_FROM = b"_ZN7planner9GoalField11setCostFromERN8bmapping14ParticleFilterEddd"        # planner::GoalField::setCostFrom(bmapping::ParticleFilter&, double, double, double)
SET_FIELD_FROM = b"_ZN10controller4MPPI16setCostFieldFromERN8bmapping14ParticleFilterEddd"    # controller::MPPI::setCostFieldFrom(bmapping::ParticleFilter&, double, double, double)
SLAM = b"_ZN8bmapping14ParticleFilter4SLAM"
APPLY_TO = b"_ZN7planner9GoalField7applyToERN10controller4MPPIEdd"


def _read(path):
    assert os.path.exists(path), "run __graft_entry__.build()"
    with open(path, "rb") as fh:
        return fh.read()


def test_node_that_owns_filter_planner_and_controller_compiles_without_a_distance_vector():
    node = _read(os.path.join(OBJ, "node_calls_nav_from_filter.o"))
    assert SET_COST_FROM in node and SET_FIELD_FROM in node and SLAM in node and APPLY_TO in node
    assert b"navCostFromDistance" not in node and b"costFieldFromDistance" not in node       # no distance field is made up or moved
    older = _read(os.path.join(OBJ, "node_calls_nav.o"))
    assert SET_COST_FROM not in older and b"navCostFromDistance" in older                    # the node of the host route is as it was
    host = _read(HOST_LIB)
    assert SET_COST_FROM in host and SET_FIELD_FROM in host


def test_scenario_u_walls_as_cells_block_the_cup_and_leave_the_way_round():
    occ = fc.scenario_u_occupancy()
    u = fc.U_FILTER
    assert occ.shape == (nr.U_GRID["nx"], nr.U_GRID["ny"]) and (u["xmin"], u["ymin"], u["resolution"]) == tuple(nr.U_GRID[k] for k in ("xmin", "ymin", "resolution"))
    assert int(np.ceil((u["xmax"] - u["xmin"]) / u["resolution"])) == 80 == int(np.ceil((u["ymax"] - u["ymin"]) / u["resolution"]))
    cost = fr.cost_from_occ(occ, u["resolution"], nr.U_R_ROBOT, nr.U_R_INFLATE, nr.U_K)
    start = nr.cell_of(**nr.U_GRID, x=0.0, y=0.0)
    assert cost[nr.U_GOAL_CELL] == 1 and cost[start] == 1
    # every cell the exact walls block is blocked by the cells too (the raster is the thicker wall)
    assert (cost[nr.scenario_u_cost() == 0] == 0).all()
    d = nr.cost_to_go(cost, nr.U_GOAL_CELL)
    assert d[start] != nr.UNREACHED and d[start] > 1.3 * 10 * (nr.U_GOAL_CELL[0] - start[0])
    assert d[nr.cell_of(**nr.U_GRID, x=0.7, y=0.0)] > d[start]


def test_scenario_u_restated_robot_arrives_over_the_rasterised_walls():
    """What the GPU behaviour test relies on: with the walls two cells thick (U_WALL_HALF = 0.03) the restated controller arrives
    within U_MAX_TICKS and never stands on a blocked cell."""
    import mppi_field_restatement as mf
    occ = fc.scenario_u_occupancy()
    cost = fr.cost_from_occ(occ, nr.U_GRID["resolution"], nr.U_R_ROBOT, nr.U_R_INFLATE, nr.U_K)
    d = nr.cost_to_go(cost, nr.U_GOAL_CELL)
    field = dict(values=nr.field(d, nr.U_GRID["resolution"], nr.U_CAP), xmin=nr.U_GRID["xmin"], ymin=nr.U_GRID["ymin"],
                 resolution=nr.U_GRID["resolution"], weight=nr.U_WEIGHT)
    state = dict(u=np.zeros((2, nr.mppi_steps(nr.U_PRM["horizon"], nr.U_PRM["dt"]))))
    visited = []

    def tick(x, noise):
        visited.append(nr.cell_of(**nr.U_GRID, x=x[0], y=x[1]))
        r = mf.mppi_new_controls_field(nr.U_PRM, state["u"], (0.0, 0.0), nr.U_WAYPOINT, x, noise, field=field)
        state["u"] = r["u"]
        return r["out"]
    ticks, least, x = nr.scenario_u_run(tick, seed=3)
    print("scenario U over the rasterised walls, restated: ticks", ticks, "least distance to the exact walls", least, "end", x)
    assert ticks is not None and ticks <= nr.U_MAX_TICKS
    assert all(c is not None and cost[c] != 0 for c in visited)
