"""levelsetpy_amd -- MI355X (gfx950) implementation of LevelSetPy's Hamilton-Jacobi time-stepping
hot path, behind the reference's own names and callback protocol:

    odeCFL1/2/3, odeCFLset  ->  termLaxFriedrichs / termRestrictUpdate
        ->  upwindFirstENO2 / ENO3 / WENO5  +  artificialDissipationGLF  +  addGhost*

All arithmetic on the path runs in hand-written HIP kernels (csrc/, C ABI in
include/hj_mi355x.h, bound with ctypes).  The package has no CPU fallback.
"""
from .utilities import *            # noqa: F401,F403
from .boundary import addGhostExtrapolate, addGhostPeriodic, addGhostAllDims   # noqa: F401
from .grids import createGrid, processGrid                                      # noqa: F401
from .init_conds import shapeCylinder, shapeSphere                              # noqa: F401
from .spatial import (upwindFirstENO2, upwindFirstENO3, upwindFirstENO3a, upwindFirstWENO5,   # noqa: F401
                      upwindFirstWENO5a, upwindFirstWENO5Intended, upwindFirstENO3aHelper,
                      set_weno5_mode, get_weno5_mode, set_eno_mode, get_eno_mode)
from .dissipation import (artificialDissipationGLF, artificialDissipationLLF,      # noqa: F401
                          artificialDissipationLLLF)
from .dynamics import DubinsVehicleRel, DoubleIntegrator, DoublePendulum4D, Plane5D, DubinsPair6D      # noqa: F401
from .user_ham import register_native_hamiltonian, NativeRegistration, RegisteredSystem, kernel_cache_stats   # noqa: F401
from .trace_ham import trace_callbacks, TraceError, set_hidim_trace, get_hidim_trace   # noqa: F401
from .term import termLaxFriedrichs, termRestrictUpdate, explain_plan           # noqa: F401
from .integration import (odeCFL1, odeCFL2, odeCFL3, odeCFLset, odeCFLget,      # noqa: F401
                          odeCFLmultipleSteps, odeCFLcallPostTimestep)
from .hji_solver import HJIPDE_solve                                            # noqa: F401
from .gradients import computeGradients                                         # noqa: F401
from .convection import termConvection                                          # noqa: F401
from .normal_reinit import termNormal, termReinit                               # noqa: F401
from .curvature import (curvatureSecond, hessianSecond, laplacianSecond,      # noqa: F401
                        centeredFirstSecond, termCurvature, termSum, termForcing)
from .trace_hessian import (termTraceHessian, termDiscount,                     # noqa: F401
                            cellMatrixMultiply, cellMatrixTrace)
from .opt_traj import computeOptTraj, find_earliest_BRS_ind                     # noqa: F401
from .query import eval_u, eval_costate, proj, augmentPeriodicData             # noqa: F401
from .surface import extract_level_set, level_set_measure, implicit_mesh       # noqa: F401
from .ttr import postTimeStepTTR, TD2TTR                                        # noqa: F401
from .rollout import computeOptTrajs                                            # noqa: F401
from .batch import HJIPDE_solve_batch                                           # noqa: F401
from .shapes import (evaluate_shape, shapeRectangleByCorners, shapeRectangleByCenter,   # noqa: F401
                     shapeHyperplane, shapeHyperplaneByPoints, shapeUnion, shapeIntersection,
                     shapeDifference, shapeComplement, sphere_of, sphere_between, compile_program_hi,
                     series, ShapeSeries)
from .decomp import sepGrid, backProject, Decomposition                          # noqa: F401
from .eikonal import signedDistance, addCRadius                                  # noqa: F401
from .resample import transformData, migrateGrid, shiftData, rotateData         # noqa: F401
from .measure import setVolume, setCompare, setBounds, truncateGrid             # noqa: F401
from . import hidim                                                              # noqa: F401
from . import stochastic                                                         # noqa: F401
from .montecarlo import computeStochTrajs, reachProbability                     # noqa: F401
from .safety import computeSafeTrajs, safeControls                              # noqa: F401
from .hidim_ham import register_hidim_hamiltonian, HidimRegistration, HidimSystem, hidim_kernel_cache_stats   # noqa: F401
from .plant import register_plant, PlantRegistration, PlantSystem, plant_kernel_cache_stats   # noqa: F401

__version__ = "0.1.0"
