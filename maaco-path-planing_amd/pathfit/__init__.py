"""pathfit: MI355X-native population-fitness engine behind the solver classes of
dvnam1605/MAACO-path-planing.  The classes keep the reference's constructor and
solve() / solve_path_planning() surface (MAACO.py:10, MPA.py:9, ga_solver.py:8,
pso.py:8, astar.py:10); the per-agent decode -> A*-stitch -> score -> update
hot path runs in hand-written HIP kernels (csrc/) behind a C-ABI
(include/pathfit.h).  No CPU fallback exists."""
from .env import FREE_SPACE, OBSTACLE, START_NODE_VAL, TARGET_NODE_VAL  # noqa: F401
from .rng import AgentRandom  # noqa: F401
from ._lib import PathfitError  # noqa: F401
from .engine import Engine, DevBuf, score_params  # noqa: F401
from .paths import CellPath  # noqa: F401
from .solvers import AStarSolver, DijkstraSolver, GASolver, PSOSolver, BasePathfinder  # noqa: F401
from .maaco import MAACO  # noqa: F401
from .maaco_batch import MAACOBatch, MaacoColony  # noqa: F401
from .mpa import MPA  # noqa: F401
from .mpa_batch import MPABatch, MpaSchool  # noqa: F401
from .ga_batch import GABatch, GaPopulation  # noqa: F401
from .pso_batch import PSOBatch, PsoSwarm  # noqa: F401
from .dist_field import DistanceField  # noqa: F401
from .nearest_field import NearestSourceField  # noqa: F401
from .smooth import PathSmoother  # noqa: F401
from .components import Components  # noqa: F401
from .clearance import Clearance, PF_CLEAR_NONE  # noqa: F401
from .cost_field import CostField  # noqa: F401
from .turn_field import TurnField  # noqa: F401
from .visibility import Visibility  # noqa: F401
from .any_angle import AnyAngle  # noqa: F401
from .spacetime import SpaceTime  # noqa: F401
from .tour import Tour  # noqa: F401
from .assignment import Assignment  # noqa: F401
from .tour_search import TourSearch  # noqa: F401
from .fleet import FleetTours  # noqa: F401
from .placement import Placement  # noqa: F401
from .cover import Coverage  # noqa: F401
