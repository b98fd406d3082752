/*
 * mrs_tg.h -- C ABI of the MI355X-native batched polynomial trajectory optimiser.
 *
 * Drop-in boundary for the numerical core of ctu-mrs/mrs_uav_trajectory_generation:
 * everything MrsTrajectoryGeneration::findTrajectory() does between building its vertices and
 * receiving the sampled states (/root/reference/src/mrs_trajectory_generation.cpp:1046-1169),
 * for a whole batch of independent paths at once.  The reference has no FFI for this path; the
 * seam is a C++ call sequence, so each entry point names the reference calls it replaces
 * (paths relative to /root/reference/, "linear_impl.h" / "nonlinear_impl.h" are
 * include/eth_trajectory_generation/impl/polynomial_optimization_{linear,nonlinear}_impl.h).
 *
 * Conventions
 *   - plain C types, caller-owned buffers, no exceptions cross the boundary;
 *   - every function returns MRS_TG_OK (0) or a negative MRS_TG_ERR_* and records a message
 *     retrievable with mrs_tg_last_error();
 *   - 4 dimensions (x, y, z, heading), 10 coefficients per polynomial in ascending powers
 *     (include/eth_trajectory_generation/polynomial.h:35-37), IEEE double throughout;
 *   - a batch is CSR over segments: path p owns segments [seg_offsets[p], seg_offsets[p+1]) and
 *     vertices [seg_offsets[p] + p, seg_offsets[p+1] + p + 1);
 *   - per-path results carry an nlopt-style status (src/mrs_trajectory_generation.cpp:1138-1149
 *     accepts >= 1 except 6, and -1).
 *   - there is NO CPU fallback: without a usable HIP device every call fails with
 *     MRS_TG_ERR_NO_DEVICE.
 */
#ifndef MRS_TG_H_
#define MRS_TG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRS_TG_ABI_VERSION 5
#define MRS_TG_N_COEFF 10
#define MRS_TG_N_DIM 4
#define MRS_TG_N_SLOT 5 /* derivative slots per vertex: position .. snap */
#define MRS_TG_MAX_SEGMENTS 256 /* longest path a plan accepts (per-path optimiser state lives in the 160 KB LDS of a CU;
                                   the reference's deviation loop ends near 30 segments) */

enum {
  MRS_TG_OK = 0,
  MRS_TG_ERR_INVALID_ARG = -1,
  MRS_TG_ERR_NO_DEVICE = -2,
  MRS_TG_ERR_HIP = -3,
  MRS_TG_ERR_UNSUPPORTED = -4,
  MRS_TG_ERR_NOMEM = -5
};

/* per-path status values (nlopt.h result codes, as consumed by the nodelet) */
enum {
  MRS_TG_STATUS_FAILURE = -1,
  MRS_TG_STATUS_INVALID_ARGS = -2, /* also: a vertex of the path leaves its POSITION unconstrained and the general solver
                                      was not asked for.  Every caller of the reference constrains the position of every
                                      vertex (src/...cpp:944, 963, 967) and the fast kernels rely on it; the general
                                      fixed / free patterns of setupConstraintReorderingMatrix (linear_impl.h:184-257)
                                      are solved under MRS_TG_FLAG_GENERAL_PATTERNS (every mode) */
  MRS_TG_STATUS_ROUNDOFF_LIMITED = -4, /* nlopt::ROUNDOFF_LIMITED, which the nodelet rejects (:1103-1106, 1146-1149).  Mellinger
                                      mode: the feasibility scaling that follows the outer loop has multiplied the path's
                                      total time by more than MRS_TG_RUNAWAY_TIME_FACTOR -- the outer loop ended on a point
                                      with a segment on the 0.01 s bound next to seconds-long neighbours, where the linear
                                      solve has a condition number of (T_max / T_min)^7 and its maxima are rounding noise
                                      (DESIGN.md section 5).  The arrays hold what was computed; it is not a trajectory
                                      to fly.  The reference returns such a path with MAXEVAL_REACHED and leaves it to the
                                      nodelet's length check (:1178-1199) to discard it */
  MRS_TG_STATUS_SUCCESS = 1,
  MRS_TG_STATUS_FTOL_REACHED = 3,
  MRS_TG_STATUS_XTOL_REACHED = 4,
  MRS_TG_STATUS_MAXEVAL_REACHED = 5,
  MRS_TG_STATUS_MAXTIME_REACHED = 6
};

/* sum of the final segment times / sum of the times the outer loop started from, above which a Mellinger result is
 * reported as MRS_TG_STATUS_ROUNDOFF_LIMITED.  Healthy paths: median 1.6, 99.9 % below 3, the largest of 8192 paths with
 * limits scaled by 0.3 ... 3 and mixed constraint patterns 18.6; runaways: 30 ... 1e10 (oracle, tests/test_oracle_runaway.py) */
#define MRS_TG_RUNAWAY_TIME_FACTOR 25.0

/* time_alloc_method (NonlinearOptimizationParameters::TimeAllocMethod,
 * include/eth_trajectory_generation/polynomial_optimization_nonlinear.h:92-100) */
enum {
  MRS_TG_TIME_ALLOC_NONE = -1,         /* fixed segment times: PolynomialOptimization::solveLinear only */
  MRS_TG_TIME_ALLOC_SQUARED_TIME = 0,  /* kSquaredTime: J_d + time_penalty (sum T)^2 + soft constraints, gradient-free */
  MRS_TG_TIME_ALLOC_RICHTER_TIME = 1,  /* kRichterTime: J_d + time_penalty sum T + soft constraints, gradient-free */
  MRS_TG_TIME_ALLOC_MELLINGER = 2,     /* kMellingerOuterLoop, the shipping default
                                          (config/private/trajectory_generation.yaml:7) */
  MRS_TG_TIME_ALLOC_SQUARED_TIME_AND_CONSTRAINTS = 3, /* kSquaredTimeAndConstraints: as 0, segment times and free
                                          end-point derivatives are the variables (nonlinear_impl.h:429-536) */
  MRS_TG_TIME_ALLOC_RICHTER_TIME_AND_CONSTRAINTS = 4  /* kRichterTimeAndConstraints: as 1, same variables */
};

enum {
  MRS_TG_FLAG_FUSED_ASSEMBLY = 1,     /* the default since ABI 2 (kept so that ABI-1 callers still say what they mean): every
                                         lane of the solve kernel forms its column of the reduced system straight from the
                                         segment times; no block is written to memory */
  MRS_TG_FLAG_MATERIALIZED_BLOCKS = 2,/* linear mode: run the assembly kernel (mrs_tg_plan_assemble: full H_i and A_i^-1 of
                                         every segment in HBM, the reference's updateSegmentTimes + constructR products) and
                                         solve from the materialised blocks */
  MRS_TG_FLAG_SHARED_DEVICE = 4,      /* a hint, results are unaffected: the caller keeps several batches in flight on this
                                         device (one context + stream each), so small batches are launched in shapes that
                                         leave wavefront slots to the other streams instead of minimising the latency of
                                         this one launch */
  MRS_TG_FLAG_GENERAL_PATTERNS = 16,  /* some vertices may leave their POSITION free (setupFromVertices takes any fixed / free
                                         pattern, linear_impl.h:184-257; the nodelet never builds such a vertex).  The fast
                                         kernels return those paths with status -2; with this flag they take a general route
                                         behind the fast kernels, in every time_alloc_method: 5 x 5 vertex blocks
                                         (mrs_tg_general.hip) for every linear solve of the pipeline, and in Mellinger mode
                                         the outer loop with that solve as its evaluation (optimize_general_kernel).  The
                                         other paths of the batch are the fast kernels' results, bit for bit.
                                         mrs_tg_solve_batch sets the flag by itself when its host copy of fixed_mask shows
                                         such a vertex; callers of the device-pointer interface say so */
  MRS_TG_FLAG_CAREFUL_COST = 8        /* Mellinger mode: paths on which a trial point's cost lost its digits in the fast
                                         evaluation (a segment on the 0.01 s bound next to long neighbours; about 0.3 % of
                                         random 10-segment paths) are run again with the cost the reference computes,
                                         0.5 c^T Q c from the coefficients (computeCost, linear_impl.h:128-141), in every
                                         evaluation.  One more kernel per call, about the duration of the outer loop
                                         itself; without the flag such a trial point is rejected where the reference may
                                         accept it.  The re-run kernel is a compile-time option
                                         (MRS_TG_WITH_CAREFUL, ON in the shipped library since ABI 4; it moves 65536 x 10
                                         from 99.9435 % to 99.9481 % agreement with the oracle): a library built without it
                                         (-DMRS_TG_WITH_CAREFUL=0) refuses the flag with MRS_TG_ERR_UNSUPPORTED, and
                                         mrs_tg_capabilities() says which one is loaded */
};

enum {
  MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS = 32 /* (ABI 4) the caller states that the position constraint of EVERY vertex is its
                                         waypoint: fixed_mask[v][0] != 0 and fixed_values[v][0][:] == waypoints[v][:], bit for
                                         bit -- what every vertex findTrajectory builds looks like
                                         (src/mrs_trajectory_generation.cpp:944, 963, 967: addConstraint(POSITION,
                                         waypoint.coords)).  `waypoints` must then be given, and kernels may read vertex
                                         positions from that compact [vertex][4] array instead of from 8 bytes out of every
                                         160 of fixed_values: the saturated-device solve (launches of >= 6144 paths) moves
                                         1.03 instead of 1.34 times its compulsory bytes.  Results are bit-identical.
                                         mrs_tg_plan_bind_solve CHECKS the statement once, on the arrays as they are at bind
                                         time, and refuses the bind with MRS_TG_ERR_INVALID_ARG if it does not hold;
                                         mrs_tg_solve_batch, which holds the three arrays in host memory, checks it on every
                                         call (O(V) on the host, before anything is uploaded or launched) and fails the same way;
                                         mrs_tg_plan_solve trusts it: the flag only changes launches that take the
                                         saturated-device kernel (>= 6144 paths per dispatch), so a statement that is false -- or
                                         has become false because the arrays of a bound solve were rewritten in place -- gives the
                                         solution of the waypoints' problem there and of the caller's problem on smaller launches.
                                         With MRS_TG_VERIFY_FLAGS=1 in the environment every mrs_tg_plan_solve re-checks the
                                         statement (a blocking check, for debugging and tests) and fails with
                                         MRS_TG_ERR_INVALID_ARG when it does not hold.  Other kernels ignore the flag */
  ,
  MRS_TG_FLAG_CONSTRAINED_SLOTS = 64  /* a HINT (results agree to rounding with and without it): beside the ends of its paths the
                                         batch may hold vertices with derivative slots constrained to zero -- stop_at waypoints --
                                         and the objective order is snap.  The min-snap launches of the large batches' kernels are
                                         compiled for position-only interior vertices (they are the benchmark configs' kernels) and
                                         hand other paths to the general steps; with the hint they run the instantiations that
                                         eliminate such vertices inside the specialised sweeps (always the case below snap).
                                         mrs_tg_solve_batch, mrs_tg_find_trajectory and mrs_tg_optimize_paths set it themselves
                                         from the masks they hold in host memory */
  ,
  MRS_TG_FLAG_REFERENCE_STATUS = 128  /* (ABI 5) Mellinger mode: the path's status is the outer loop's own stopping reason, as in
                                         the reference -- the product's runaway rule (MRS_TG_STATUS_ROUNDOFF_LIMITED when the
                                         feasibility scaling multiplied the total time by more than MRS_TG_RUNAWAY_TIME_FACTOR)
                                         is switched off.  For callers that apply the reference's own answer to a runaway, the
                                         length check against the Baca estimate (src/...cpp:1178-1199): mrs_tg_find_trajectory and
                                         mrs_tg_optimize_paths set the flag themselves, and ONLY where the upper side of that check
                                         really runs -- the seam when it samples (sampling_dt > 0, samples_out given) and
                                         max_trajectory_len_factor > 0, the policy when its max_trajectory_len_factor > 0.
                                         Elsewhere (an mrs_tg_options opt{} has both factors 0) nothing of the reference would
                                         answer a runaway, so the product's rule stays on and the path is rejected by its code,
                                         -4.  The rule measures against the Euclidean
                                         estimate, which is 0.01-0.03 s for waypoints a few centimetres apart: such a path is
                                         stretched 25-fold by a perfectly healthy scaling, and the reference never checks a
                                         trajectory shorter than one second.  Coefficients, times and samples are the same bits
                                         with and without the flag */
  ,
  MRS_TG_FLAG_REFINE = 256            /* every mode: after the final linear solve, each path with status > 0 is refined at its
                                         returned segment times (mrs_tg_refine.hip): vertex derivatives held in double-double,
                                         the residual of the free slots formed in double-double from exact unit-time constants,
                                         corrections solved in double (one factorisation, at most 3 steps, a step kept only if
                                         it lowered the residual), coefficients formed in double-double and rounded once, the
                                         cost recomputed.  R_pp's condition number grows like (T_max / T_min)^7 between
                                         neighbouring segments; without the flag such a path (a 0.18 s segment between 4 s ones)
                                         is 1e-8 off, with it 1e-11 or better.  What is refined: coeffs and cost.  What is not:
                                         segment times, status, and the time-allocation search's own evaluations -- times and
                                         status are bit-identical to the same call without the flag and without sampling;
                                         samples are taken from the refined coefficients.  Cost: one more kernel per call,
                                         12-31 times the solve it follows (10240 x 10: 446 us after a 31 us solve), and a
                                         workspace of 2080 bytes per path per vertex of the plan's longest path, kept by the plan
                                         (65536 x 10: 1.5 GB).  Refused with MRS_TG_ERR_UNSUPPORTED by
                                         mrs_tg_bound_solve_launch_group */
};

/* mrs_tg_capabilities(): what this build of the library contains beyond the mandatory surface */
enum {
  MRS_TG_CAP_CAREFUL_COST = 1, /* MRS_TG_FLAG_CAREFUL_COST is honoured (optimize_careful_kernel is built in) */
  MRS_TG_CAP_FUTURE_PATHS = 2, /* the initial condition of paths stamped in the future: mrs_tg_prepare_initial_condition and
                                  mrs_tg_splice_prediction are exported */
  MRS_TG_CAP_REFINE = 4,       /* MRS_TG_FLAG_REFINE is honoured (refine_kernel is built in) */
  MRS_TG_CAP_GRADIENT = 8,     /* mrs_tg_plan_solve_vjp is exported: the backward pass of the fixed-times solve */
  MRS_TG_CAP_MAXIMA_GRADIENT = 16, /* mrs_tg_plan_segment_maxima_vjp is exported: the backward pass of the segment maxima */
  MRS_TG_CAP_SAMPLE_GRADIENT = 32, /* mrs_tg_plan_sample_states_vjp and mrs_tg_plan_sample are exported: the backward pass of
                                      the sampler */
  MRS_TG_CAP_EVALUATE = 64,        /* mrs_tg_plan_evaluate and mrs_tg_plan_evaluate_vjp are exported: the state at caller-given
                                      times and its backward pass */
  MRS_TG_CAP_DEVIATION = 128,      /* mrs_tg_plan_path_deviation and mrs_tg_plan_path_deviation_vjp are exported: the deviation
                                      of the samples from the waypoint polyline and its backward pass */
  MRS_TG_CAP_ESTIMATE_GRADIENT = 256, /* mrs_tg_plan_estimate_times and mrs_tg_plan_estimate_times_vjp are exported: the Euclidean
                                         segment-time estimate as a plan step and its backward pass */
  MRS_TG_CAP_WAYPOINT_PASSAGE = 512,  /* mrs_tg_plan_waypoint_passage and mrs_tg_plan_waypoint_passage_vjp are exported: where the
                                         samples pass the requested waypoints (index, miss distance, foot point) and its
                                         backward pass */
  MRS_TG_CAP_BACA = 1024,             /* mrs_tg_plan_estimate_times_baca, mrs_tg_plan_estimate_times_baca_vjp and
                                         mrs_tg_plan_length_gate are exported: the Baca segment-time estimate as a plan step, its
                                         backward pass, and the length gate on its total */
  MRS_TG_CAP_FALLBACK_SAMPLE = 2048,  /* mrs_tg_plan_unwrap_headings, mrs_tg_plan_fallback_sample and
                                         mrs_tg_plan_fallback_sample_vjp are exported: the fallback sampler (findTrajectoryFallback)
                                         as a plan step, its backward pass, and the heading unwrap in front of its clock */
  MRS_TG_CAP_PATH_EDIT = 4096,        /* mrs_tg_plan_preprocess_path, mrs_tg_plan_insert_midpoints and mrs_tg_plan_path_edit_vjp
                                         are exported: the two steps that change the number of waypoints of a path (preprocessPath's
                                         thinning, the mid-points of unsafe segments) and their one backward pass */
  MRS_TG_CAP_TRAVEL_HEADING = 8192,   /* mrs_tg_plan_travel_heading and mrs_tg_plan_travel_heading_vjp are exported: the heading
                                         along the direction of travel (override_heading_atan2) as a plan step and its backward
                                         pass */
  MRS_TG_CAP_INITIAL_CONDITION = 16384, /* mrs_tg_plan_initial_condition, mrs_tg_plan_prepend_initial_condition,
                                         mrs_tg_plan_splice_prediction and their three backward passes are exported: where a
                                         trajectory starts (prepareInitialCondition), the waypoint put in front of the request
                                         and the prediction in front of a trajectory from the future, as plan steps */
  MRS_TG_CAP_REQUEST = 32768,           /* mrs_tg_plan_request_vertices, mrs_tg_plan_request_limits and their two backward passes
                                         are exported: the vertices and the limits findTrajectory derives from a request, as plan
                                         steps */
  MRS_TG_CAP_MUTUAL_CLEARANCE = 65536,  /* mrs_tg_plan_mutual_clearance and mrs_tg_plan_mutual_clearance_vjp are exported: how close
                                         the paths of one group (a swarm) come to each other at common steps, the nearest
                                         neighbour's index, and the backward pass */
  MRS_TG_CAP_OBSTACLE_CLEARANCE = 131072, /* mrs_tg_plan_obstacle_clearance and mrs_tg_plan_obstacle_clearance_vjp are exported: the
                                         signed distance of every row to the nearest sphere or point of the path's obstacle set,
                                         that obstacle's index, and the backward pass */
  MRS_TG_CAP_FIELD_CLEARANCE = 262144,  /* mrs_tg_plan_field_clearance and mrs_tg_plan_field_clearance_vjp are exported: the
                                         trilinear interpolant of a voxel grid of signed distances at every row, its cell, the
                                         field's gradient, and the backward pass */
  MRS_TG_CAP_FIELD_FROM_OCCUPANCY = 524288, /* mrs_tg_field_from_occupancy is exported: that grid of (signed) distances built on
                                         the device from an occupancy grid by an exact Euclidean distance transform */
  MRS_TG_CAP_FIELD_UPDATE_REGION = 1048576 /* mrs_tg_field_update_query and mrs_tg_field_update_region are exported: that grid
                                         brought up to date after the occupancy changed inside a box, in the full rebuild's bits */
};

/* mrs_tg_plan_request_limits' flags_dev: what the request asks of its limits */
enum {
  MRS_TG_REQ_OVERRIDE = 1,      /* override_constraints: the six override values replace the horizontal and vertical limits */
  MRS_TG_REQ_RELAX_HEADING = 2  /* relax_heading: the three heading limits become (double)FLT_MAX */
};

/* mrs_tg_plan_request_limits' branch_out_dev: which branches the limits of a path took, as bits; what its backward pass is
 * driven by */
enum {
  MRS_TG_LIM_OVERRIDDEN = 1,       /* the override replaced the six values */
  MRS_TG_LIM_OVERRIDE_REFUSED = 2, /* the override was asked for and refused: the state is not strictly inside it (:1001-1008) */
  MRS_TG_LIM_RELAXED = 4,          /* the heading limits were relaxed */
  MRS_TG_LIM_V_DESCENDING = 8,     /* the vertical speed of the constraints is the descending one (strictly smaller) */
  MRS_TG_LIM_A_DESCENDING = 16,    /* ... the vertical acceleration */
  MRS_TG_LIM_J_DESCENDING = 32,    /* ... the vertical jerk */
  MRS_TG_LIM_FALLBACK = 64         /* findTrajectoryFallback's variant: no can_change test, the two factors applied */
};

/* mrs_tg_plan_initial_condition's decision_out_dev: what prepareInitialCondition and the first-waypoint rule decided for a
 * path, as bits.  One of FROM_TRACKER, FROM_UAV, FROM_PREDICTION is set exactly where PREPEND is; FROM_FUTURE goes with
 * FROM_PREDICTION; DROP_FIRST stands for itself; INVALID stands alone. */
enum {
  MRS_TG_IC_PREPEND = 1,          /* the path has an initial condition: a waypoint goes in front, the state block holds it */
  MRS_TG_IC_FROM_FUTURE = 2,      /* sample at 0.2 s and splice the prediction in front afterwards */
  MRS_TG_IC_DROP_FIRST = 4,       /* erase the first requested waypoint before prepending (:650-655) */
  MRS_TG_IC_FROM_TRACKER = 8,     /* the state is the tracker command */
  MRS_TG_IC_FROM_UAV = 16,        /* ... the UAV state lifted by the takeoff height, derivatives zero (before takeoff) */
  MRS_TG_IC_FROM_PREDICTION = 32, /* ... row k of the prediction */
  MRS_TG_IC_INVALID = 64          /* a NaN time offset, a NaN age of a tracker command that is present, or n_pred outside
                                     [0, pred_capacity]: no initial condition, the caller fails the path */
};

/* mrs_tg_plan_estimate_times_vjp's term_out_dev: the term of the estimate a segment's time came from */
enum {
  MRS_TG_ESTIMATE_TERM_HORIZONTAL = 0, /* h / v_h: |inclination| <= atan2(v_v, v_h) */
  MRS_TG_ESTIMATE_TERM_VERTICAL = 1,   /* |dz| / v_v: steeper than that */
  MRS_TG_ESTIMATE_TERM_FLOOR = 2,      /* the forward took 0.01 */
  MRS_TG_ESTIMATE_TERM_HEADING = 3     /* 1.5 (t_vel + t_acc) exceeded the distance term, strictly */
};

/* mrs_tg_plan_estimate_times_baca_vjp's flags_out_dev: the branches of the Baca estimate a segment's time took, as bits */
enum {
  MRS_TG_BACA_V_VERTICAL = 1,       /* |inclination| > atan2(v_v, v_h): v_max = |v_v / sin|, else |v_h / cos| */
  MRS_TG_BACA_A_VERTICAL = 2,       /* the same decision for the acceleration limits */
  MRS_TG_BACA_J_VERTICAL = 4,       /* and for the jerk limits */
  MRS_TG_BACA_T1_CAPPED = 8,        /* the acceleration time in front was sqrt(2 distance / a_max), the smaller */
  MRS_TG_BACA_T2_CAPPED = 16,       /* the acceleration time behind was */
  MRS_TG_BACA_DOT1_CLAMPED = 32,    /* the cosine of the corner in front was negative: its coefficient is the constant 1 */
  MRS_TG_BACA_DOT2_CLAMPED = 64,    /* the cosine of the corner behind was */
  MRS_TG_BACA_FLOOR = 128,          /* the forward took 0.01 */
  MRS_TG_BACA_HEADING = 256,        /* 1.5 (t_vel + t_acc) exceeded all of that, strictly */
  MRS_TG_BACA_HEADING_CRUISE = 512, /* the heading term's `reduced >= 0` branch */
  MRS_TG_BACA_HEADING_ACC = 1024    /* ang > pi/4 */
};

typedef struct mrs_tg_options {
  int32_t derivative_to_optimize; /* 2 acceleration, 3 jerk, 4 snap (src/...cpp:904-919) */
  int32_t time_alloc_method;      /* MRS_TG_TIME_ALLOC_* */
  int32_t estimate_times;         /* != 0: initial times from estimateSegmentTimes (src/...cpp:1046,
                                     vertex.cpp:491-565); 0: use seg_times_inout as given */
  int32_t max_iterations;         /* nlopt maxeval (nonlinear_impl.h:73; param max_iterations) */
  double f_rel, f_abs;            /* nlopt ftol (src/...cpp:884; nonlinear.h:42-46) */
  double x_rel, x_abs;            /* nlopt xtol (src/...cpp:885; nonlinear.h:48-54) */
  double sampling_dt;             /* > 0: sample the result (sampleWholeTrajectory, src/...cpp:1169) */
  int32_t sample_capacity;        /* samples_out holds this many samples per path */
  int32_t flags;                  /* MRS_TG_FLAG_* */
  /* gradient-free modes 0 / 1 / 3 / 4 only (objectiveFunctionTime[AndConstraints], nonlinear_impl.h:568-614, 651-722) */
  double time_penalty;            /* param time_penalty (config/private/trajectory_generation.yaml:4) */
  double soft_constraint_weight;  /* param soft_constraints_weight (:6) */
  int32_t use_soft_constraints;   /* param soft_constraints_enabled (:5) */
  int32_t reserved_;
  double initial_stepsize_rel;    /* 0.1 (src/...cpp:893) */
  double max_time_s;              /* nlopt maxtime (src/...cpp:899: 2 * 0.95 * timeLeft()); <= 0: none.  The time-allocation
                                     search of a path that is still running when the budget has passed stops at its last
                                     evaluated point with MRS_TG_STATUS_MAXTIME_REACHED (checked once per objective
                                     evaluation against the device's constant-rate clock; the budget starts when the
                                     search kernel starts, for mrs_tg_solve_batch minus the host time already spent in
                                     the call) */
  /* (ABI 5) mrs_tg_find_trajectory only -- the temporal sanity check of findTrajectory (src/...cpp:1178-1199): a sampled
   * trajectory longer than one second whose length n_samples * sampling_dt exceeds max_trajectory_len_factor times, or falls
   * below min_trajectory_len_factor times, the path's Baca estimate (estimateSegmentTimesBaca summed, :1048-1056) is
   * discarded.  Defaults 3.0 / 0.33 (config/public/trajectory_generation.yaml:35-36); <= 0 switches that side off.  The
   * batched solve calls ignore both (they are handed vertices, not a path); mrs_tg_optimize_paths uses the pair in
   * mrs_tg_policy_options */
  double max_trajectory_len_factor, min_trajectory_len_factor;
} mrs_tg_options;

typedef struct mrs_tg_ctx mrs_tg_ctx;
typedef struct mrs_tg_plan mrs_tg_plan;

/* ---- context ------------------------------------------------------------------------------- */

/* Bind a context to HIP device `device_ordinal`.  One context per thread/stream; re-entrant
 * across contexts.  Replaces the construction of PolynomialOptimizationNonLinear<10>
 * (src/mrs_trajectory_generation.cpp:1064). */
int mrs_tg_create(int device_ordinal, mrs_tg_ctx** ctx_out);
void mrs_tg_destroy(mrs_tg_ctx* ctx);
const char* mrs_tg_last_error(const mrs_tg_ctx* ctx); /* ctx may be NULL: last global error */
int mrs_tg_abi_version(void);
int mrs_tg_capabilities(void); /* MRS_TG_CAP_* bits (ABI 4) */
void mrs_tg_default_options(mrs_tg_options* opt);

/* Launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) instead of
 * the context's own stream.  NULL means HIP's null (default) stream, which is what torch uses unless a
 * side stream is current.  mrs_tg_reset_stream() goes back to the context's own stream. */
int mrs_tg_set_stream(mrs_tg_ctx* ctx, void* hip_stream);
int mrs_tg_reset_stream(mrs_tg_ctx* ctx);
int mrs_tg_synchronize(mrs_tg_ctx* ctx);

/* ---- several devices -------------------------------------------------------------------------- */

/* A set of contexts, one per entry of `device_ordinals` (an ordinal may repeat: two contexts on one GPU), for
 * mrs_tg_multi_solve_batch.  The reference handles one path per request on one worker thread
 * (src/mrs_trajectory_generation.cpp:1064-1083, 1513); paths are independent, so a batch shards over the devices with no
 * exchange between them. */
typedef struct mrs_tg_multi mrs_tg_multi;
int mrs_tg_create_multi(const int* device_ordinals, int n_devices, mrs_tg_multi** multi_out);
void mrs_tg_destroy_multi(mrs_tg_multi* multi);
int mrs_tg_multi_n_devices(const mrs_tg_multi* multi);
mrs_tg_ctx* mrs_tg_multi_context(mrs_tg_multi* multi, int index); /* the context of device `index` (owned by `multi`) */
/* Which device solves which path: shard_out[p] in [0, n_devices).  Uniform batches are cut into contiguous ranges whose
 * sizes differ by at most one; ragged batches are balanced on the segment count (longest path first onto the least
 * loaded device). */
int mrs_tg_multi_shard(const mrs_tg_multi* multi, int32_t n_paths, const int32_t* seg_offsets, int32_t* shard_out);
/* mrs_tg_solve_batch over all devices of `multi`: same arguments, same results (every path is solved by exactly the
 * kernels a single-device call would run on it).  One host thread per device solves its shard from / into the caller's
 * buffers; returns the first error of any shard (mrs_tg_multi_last_error). */
int mrs_tg_multi_solve_batch(mrs_tg_multi* multi, int32_t n_paths, const int32_t* seg_offsets, const double* waypoints,
                             const uint8_t* fixed_mask, const double* fixed_values, const double* limits,
                             const mrs_tg_options* opt, double* seg_times_inout, double* coeffs_out, int32_t* status_out,
                             double* cost_out, int32_t* n_samples_out, double* samples_out);
const char* mrs_tg_multi_last_error(const mrs_tg_multi* multi);

/* ---- one-call host interface ---------------------------------------------------------------- */

/* Host buffers in, host buffers out; blocking.  A batch of one path reproduces the nodelet's call.
 * Replaces: estimateSegmentTimes (src/...cpp:1046), setupFromVertices (:1065; linear_impl.h:62-106),
 * the 12 addMaximumMagnitudeConstraint calls (:1067-1081, folded into `limits`), optimize() (:1083;
 * nonlinear_impl.h:90-234,336-408), getTrajectory (:1163) and sampleWholeTrajectory (:1169).
 *
 *   waypoints      [sum V][4]      x, y, z, heading (already unwrapped as at src/...cpp:935)
 *   fixed_mask     [sum V][5]      != 0: derivative k of the vertex is constrained (Vertex::addConstraint)
 *   fixed_values   [sum V][5][4]   the constrained values (ignored where the mask is 0)
 *   limits         [n_paths][9]    {v,a,j} x {horizontal, vertical, heading}: index 3*(k-1)+group;
 *                                  a heading limit >= FLT_MAX means relax_heading (src/...cpp:1030-1038)
 *   seg_times_inout[sum S]         in: segment times (unless estimate_times); out: final times
 *   coeffs_out     [sum S][4][10]
 *   status_out     [n_paths]       nlopt-style code;  cost_out [n_paths] J_d (computeCost) -- may be NULL
 *   n_samples_out  [n_paths], samples_out [n_paths][sample_capacity][4] (x, y, z, heading wrapped to
 *                  (-pi, pi] as the nodelet reads it, src/...cpp:1582-1599) -- may be NULL when
 *                  sampling_dt <= 0.  n_samples_out reports the count the reference would produce when it
 *                  fits; a longer trajectory is reported as sample_capacity + 1 (only the first
 *                  sample_capacity samples are written) -- size the capacity from the length the caller
 *                  would still accept (the nodelet's max_trajectory_len_factor check, src/...cpp:1178-1186).
 */
int mrs_tg_solve_batch(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* seg_offsets, const double* waypoints,
                       const uint8_t* fixed_mask, const double* fixed_values, const double* limits,
                       const mrs_tg_options* opt, double* seg_times_inout, double* coeffs_out, int32_t* status_out,
                       double* cost_out, int32_t* n_samples_out, double* samples_out);

/* Pinned host memory for the arrays of mrs_tg_solve_batch, mrs_tg_multi_solve_batch and mrs_tg_find_trajectory.  The call
 * keeps one device block and one pinned staging block per context and moves each array the cheapest way its location
 * allows: an array in pinned memory (from mrs_tg_host_alloc, registered with mrs_tg_host_register, or any block of
 * hipHostMalloc) is read / written by the DMA engines in place; small pageable arrays are packed into the staging block
 * and travel as ONE copy per direction; large pageable arrays go through hipMemcpyAsync on the caller's pages.  A host that
 * calls in a loop (the nodelet's worker: std::vector outputs it re-uses) gets the PCIe rate by allocating its in / out
 * arrays here once.  mrs_tg_host_register pins an existing allocation until mrs_tg_host_unregister: the caller must
 * unregister before it frees or reallocates the block. */
int mrs_tg_host_alloc(size_t bytes, void** ptr_out);
void mrs_tg_host_free(void* ptr);
int mrs_tg_host_register(void* ptr, size_t bytes);
int mrs_tg_host_unregister(void* ptr);

/* ---- plan interface: analysis once, device-resident data, asynchronous ----------------------- */

/* Analyse the batch structure (host seg_offsets): sorts paths by segment count, sizes the
 * workspace, uploads the CSR structure.  Corresponds to the structural half of setupFromVertices
 * (setupConstraintReorderingMatrix, linear_impl.h:184-257). */
int mrs_tg_plan_create(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* seg_offsets_host, mrs_tg_plan** plan_out);
void mrs_tg_plan_destroy(mrs_tg_plan* plan);
int32_t mrs_tg_plan_n_paths(const mrs_tg_plan* plan);
int32_t mrs_tg_plan_n_segments(const mrs_tg_plan* plan);
int32_t mrs_tg_plan_max_segments(const mrs_tg_plan* plan);
/* order_out[q] = index of the path processed in position q (paths sorted by segment count, longest
 * first, stable).  The materialised blocks below are laid out by position q. */
int mrs_tg_plan_get_order(const mrs_tg_plan* plan, int32_t* order_out);

/* The Hessian / mapping-block assembly kernel on its own: for every segment of every path
 * H_i = A_i^-T Q_i A_i^-1 and A_i^-1, both full 10x10 f64 (updateSegmentTimes linear_impl.h:289-304
 * + the block products of constructR :317-320).  seg_times_dev [sum S] (CSR order).
 * Output layout ("slot-major SoA", stated in DESIGN.md): element (r, c) of the block of segment j of
 * the path at position q lives at  ((j * 100 + r * 10 + c) * n_paths + q);  each output holds
 * max_segments * 100 * n_paths doubles; slots j >= S_q are left untouched. Asynchronous. */
int mrs_tg_plan_assemble(mrs_tg_plan* plan, int32_t derivative_to_optimize, const double* seg_times_dev,
                         double* H_dev, double* Ainv_dev);
/* Bytes needed for each of H_dev / Ainv_dev. */
size_t mrs_tg_plan_block_bytes(const mrs_tg_plan* plan);

/* Same contract as mrs_tg_solve_batch but every pointer is DEVICE memory (inputs already resident in
 * HBM) and the call is asynchronous on the context's stream.  samples/cost pointers may be NULL. */
int mrs_tg_plan_solve(mrs_tg_plan* plan, const double* waypoints_dev, const uint8_t* fixed_mask_dev,
                      const double* fixed_values_dev, const double* limits_dev, const mrs_tg_options* opt,
                      double* seg_times_inout_dev, double* coeffs_out_dev, int32_t* status_out_dev,
                      double* cost_out_dev, int32_t* n_samples_out_dev, double* samples_out_dev);

/* A solve with its arguments fixed once: mrs_tg_bound_solve_launch(b) enqueues what mrs_tg_plan_solve would with the
 * arguments given here (options copied; the device buffers must stay where they are).  For a server that keeps several
 * batches in flight and re-issues the same solve step after step: the per-step host cost is one pointer. */
typedef struct mrs_tg_bound_solve mrs_tg_bound_solve;
int mrs_tg_plan_bind_solve(mrs_tg_plan* plan, const double* waypoints_dev, const uint8_t* fixed_mask_dev,
                           const double* fixed_values_dev, const double* limits_dev, const mrs_tg_options* opt,
                           double* seg_times_inout_dev, double* coeffs_out_dev, int32_t* status_out_dev, double* cost_out_dev,
                           int32_t* n_samples_out_dev, double* samples_out_dev, mrs_tg_bound_solve** bound_out);
int mrs_tg_bound_solve_launch(mrs_tg_bound_solve* bound);
void mrs_tg_bound_solve_destroy(mrs_tg_bound_solve* bound);
/* The issue loop of a host that keeps several batches in flight: launch k = 0 .. n_launches-1 goes to bound[k % n_bound]
 * (one bound solve per context + stream).  Stops at the first error and returns its code (mrs_tg_last_error of that
 * solve's context has the text). */
int mrs_tg_bound_solve_launch_many(mrs_tg_bound_solve* const* bound, int32_t n_bound, int32_t n_launches);
/* The same loop on n_threads host threads (the caller + helper threads of the library, created on first use) -- a runtime
 * launch costs the host 3.5-4.5 us, more than four concurrent 10 us kernels take to retire one, so one issuing thread
 * bounds a host with four batches in flight.  The bound solves are partitioned by CONTEXT: all solves of one context are
 * issued by the same thread (a context is driven by one thread at a time), in their order within the run; n_threads is
 * lowered to the number of distinct contexts.  Concurrent callers are served one run after the other.  The helpers spin
 * for 2 ms after a run before they go to sleep.  Returns when every launch has been issued (not finished). */
int mrs_tg_bound_solve_launch_many_mt(mrs_tg_bound_solve* const* bound, int32_t n_bound, int32_t n_launches,
                                      int32_t n_threads);
/* The same loop with consecutive launches packed into one dispatch: launch k still solves bound[k % n_bound], but a run of
 * consecutive launches whose bound solves share a PLAN (one batch structure, one context and stream; the solves differ in
 * their input / output arrays) goes out as a single kernel, on that plan's stream, whose workgroups are divided among the
 * batches (at most 16, and never the same bound solve twice).  bound = [A0, A1, B0, B1] with A*, B* bound to two plans issues
 * (A0 A1), (B0 B1), (A0 A1), ... alternately on the two plans' streams.  A launch costs the host 3 us and a 1024-path solve
 * occupies a quarter of an MI355X for 9 us: a host that issues them one by one is the bottleneck of a short run.
 * Requirements (else MRS_TG_ERR_UNSUPPORTED with a message): fixed segment times, the default solve (no
 * MRS_TG_FLAG_MATERIALIZED_BLOCKS / _GENERAL_PATTERNS), no sampling, batches the default solve takes.  The results are those
 * of mrs_tg_bound_solve_launch_many, bit for bit. */
int mrs_tg_bound_solve_launch_group(mrs_tg_bound_solve* const* bound, int32_t n_bound, int32_t n_launches);
/* Building blocks of the outer loop, exposed for parity tests (device pointers, asynchronous):
 * J_d and the h = 0.1 forward-difference gradient at the given times
 * (getCostAndGradientMellinger, nonlinear_impl.h:257-333): cost_out_dev [n_paths], grad_out_dev [sum S]. */
int mrs_tg_plan_cost_gradient(mrs_tg_plan* plan, int32_t derivative_to_optimize, const uint8_t* fixed_mask_dev,
                              const double* fixed_values_dev, const double* seg_times_dev, double* cost_out_dev,
                              double* grad_out_dev);
/* Per-segment maxima of |p^(k)| for k = 1..3 and the groups {x,y}, {z}, {heading}
 * (Trajectory::computeMaxDerivatives*, trajectory.cpp:422-565): maxima_out_dev [sum S][3][3] indexed
 * [segment][k-1][group]. */
int mrs_tg_plan_segment_maxima(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev,
                               double* maxima_out_dev);
/* Backward pass of the fixed-times solve (MRS_TG_CAP_GRADIENT; vjp_kernel): given what a
 * mrs_tg_plan_solve with time_alloc_method = MRS_TG_TIME_ALLOC_NONE returned for (fixed_mask, fixed_values, seg_times) --
 * coeffs_dev [sum S][4][10] and status_dev [n_paths] -- and the gradient of a loss L with respect to the coefficients
 * (grad_coeffs_dev [sum S][4][10]) and the cost (grad_cost_dev [n_paths]), writes dL/dfixed_values
 * (grad_fixed_values_out_dev [sum V][5][4]; 0 on the free slots) and dL/dseg_times (grad_seg_times_out_dev [sum S]).  The
 * exact chain rule of the linear QP at the returned solution: the free slots of the vertices are those the coefficients hold,
 * one adjoint solve with the same masked R_pp per path and dimension (a vanishing pivot leaves its multiplier at 0).  Any
 * fixed / free pattern; derivative_to_optimize 0 .. 4 as for the solve.  At least one upstream array and one output must be
 * given; a NULL upstream counts as zero, a NULL output is not written.  A path with status <= 0 gets zeros in all of its
 * output rows.  Not differentiated here: time allocation, sampling, and the maxima that the feasibility scaling and the
 * limits rest on (those: mrs_tg_plan_segment_maxima_vjp).  Deterministic (no atomics).
 * Device pointers in the caller's CSR order, asynchronous on the context's stream; per-lane factors in the plan's workspace
 * (1440 bytes per path per vertex of the plan's longest path). */
int mrs_tg_plan_solve_vjp(mrs_tg_plan* plan, int32_t derivative_to_optimize, const uint8_t* fixed_mask_dev,
                          const double* fixed_values_dev, const double* seg_times_dev, const double* coeffs_dev,
                          const int32_t* status_dev, const double* grad_coeffs_dev, const double* grad_cost_dev,
                          double* grad_fixed_values_out_dev, double* grad_seg_times_out_dev);
/* Backward pass of the segment maxima (MRS_TG_CAP_MAXIMA_GRADIENT; segment_maxima_vjp_kernel): given
 * the gradient of a loss L with respect to what mrs_tg_plan_segment_maxima returns for (coeffs_dev, seg_times_dev) --
 * grad_maxima_dev [sum S][3][3], required -- writes dL/dcoeffs (grad_coeffs_out_dev [sum S][4][10]), dL/dseg_times
 * (grad_seg_times_out_dev [sum S]) and the maximiser t* in seconds of every entry (argmax_out_dev [sum S][3][3]); a NULL
 * output is not written, at least one must be given.  By the envelope theorem, for the entry (k, group) with maximiser t*
 * and u = p^(k)(t*) / |p^(k)(t*)|: dM/dc[dim][j] = u_dim j!/(j-k)! t*^(j-k) (j >= k, dim in the group) and dM/dT =
 * u . p^(k+1)(T) if t* = T, else 0.  Non-smooth cases:
 *   winner -- t* is the candidate of the forward's own search that produced its value: the first, in the search's
 *     evaluation order, whose magnitude equals the maximum; on a tie (two equal peaks) the result is that winner's one-sided
 *     gradient (an element of the Clarke subdifferential), the same bits on every call;
 *   refinement -- an interior winner is polished by at most 4 Newton steps on d|p^(k)|^2/dt, kept only if it stays in the
 *     winner's grid cell and within 2^-20 of the segment's length from the winner, is a maximum there and the magnitude did
 *     not fall beyond rounding (else the winner itself); end points are not refined; the forward's values are never changed;
 *   degenerate -- a zero maximum contributes 0; an entry whose upstream is exactly 0 contributes exactly 0; a segment with
 *     T <= 0 or a non-finite T or coefficient gets zero rows (and t* = 0).
 * The 9 entries of a segment are summed in a fixed order: deterministic (no atomics, no workspace).  Device pointers in CSR
 * order, asynchronous on the context's stream. */
int mrs_tg_plan_segment_maxima_vjp(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev,
                                   const double* grad_maxima_dev, double* grad_coeffs_out_dev, double* grad_seg_times_out_dev,
                                   double* argmax_out_dev);
/* sampleWholeTrajectory with every field of the sampled state (sampleTrajectoryInRange, trajectory_sampling.cpp:49-104:
 * five evaluateRange passes over the same accumulate-and-carry walk, trajectory.cpp:93-151): for the trajectories given by
 * coeffs_dev [sum S][4][10] and seg_times_dev [sum S], states_out_dev [n_paths][sample_capacity][MRS_TG_STATE_ORDERS][4]
 * holds per sample the derivative orders 0..4 of (x, y, z, heading) -- position_W / velocity_W / acceleration_W / jerk_W /
 * snap_W in the first three columns, yaw (wrapped to (-pi, pi] as setFromYaw's quaternion round trip does), yaw rate and
 * yaw acceleration in the fourth; time_from_start of sample i is i * sampling_dt.  n_samples_out_dev [n_paths] as for the
 * solve calls (capacity + 1 = more samples than fit).  The solve calls' own samples_out (positions and heading, all the
 * nodelet reads: src/mrs_trajectory_generation.cpp:1582-1599) are order 0 of this, bit for bit.  Device pointers,
 * asynchronous on the context's stream. */
/* How many paths of the plan's most recent Mellinger solve with MRS_TG_FLAG_CAREFUL_COST had a trial point whose
 * by-product cost lost its digits and were run again.  Blocks until that solve has finished. */
int mrs_tg_plan_careful_count(mrs_tg_plan* plan, int32_t* count_out);
#define MRS_TG_STATE_ORDERS 5
int mrs_tg_plan_sample_states(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev, double sampling_dt,
                              int32_t sample_capacity, int32_t* n_samples_out_dev, double* states_out_dev);

/* The positions + heading sampler on its own (what the solve calls write to samples_out when sampling_dt > 0): the same
 * arguments as mrs_tg_plan_sample_states with samples_out_dev [n_paths][sample_capacity][4], order 0 of the states bit for
 * bit at a fifth of the stores. */
int mrs_tg_plan_sample(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev, double sampling_dt,
                       int32_t sample_capacity, int32_t* n_samples_out_dev, double* samples_out_dev);
/* Backward pass of the sampler (MRS_TG_CAP_SAMPLE_GRADIENT; sample_vjp_kernel): given the gradient of
 * a loss L with respect to the samples -- grad_states_dev [n_paths][sample_capacity][n_orders][4], n_orders = 1 (the
 * upstream of mrs_tg_plan_sample / the solve calls' samples_out) or MRS_TG_STATE_ORDERS (of mrs_tg_plan_sample_states) --
 * writes dL/dcoeffs (grad_coeffs_out_dev [sum S][4][10]) and dL/dseg_times (grad_seg_times_out_dev [sum S]), and, with or
 * without an upstream, what the gradient is taken at: per sample the segment (index within its path) and the time in that
 * segment in seconds of the forward's own walk (sample_segment_out_dev / sample_time_out_dev [n_paths][sample_capacity];
 * entries at or beyond a path's sample count are not written) and the counts (n_samples_out_dev [n_paths], as the forward
 * reports them).  Sample k of segment i_k at the time t_k = k dt - sum_{i < i_k} T_i contributes
 *   dL/dc[i_k][dim][j] += sum_{o <= min(j, n_orders-1)} G[k][o][dim] j!/(j-o)! t_k^(j-o)
 *   dL/dT_i            -= sum_{o, dim} G[k][o][dim] p_dim^(o+1)(t_k)      for every segment i < i_k.
 * What is not smooth, and what the call does there:
 *   sample count and segment membership -- piecewise constant in the times: the gradient is that of the walk the forward
 *     took, n and i_k held fixed (positions are continuous across a segment boundary; the one true discontinuity of a loss on
 *     positions is the appearance of a new last sample when the total time crosses a multiple of dt);
 *   the floating-point walk -- t_k is a chain of rounded additions and carries; it is differentiated as its exact
 *     counterpart, dt_k/dT_i = -1 for the segments in front of the sample's own and 0 otherwise;
 *   heading wrap -- derivative 1, at the seam the one-sided value;
 *   overflow -- when the forward reports sample_capacity + 1, the first sample_capacity samples exist and contribute;
 *   rows of the upstream at or beyond a path's sample count are never read;
 *   degenerate -- a path whose total time is not a number has no samples and gets zero rows; with status_dev, a path with
 *     status <= 0 gets zero rows whatever its coefficients hold; a segment without a sample gets zero coefficient rows and
 *     still its time gradient from the samples behind it.
 * At least one output must be given, the two gradients need grad_states_dev; every output element that belongs to the plan
 * is written exactly once (zeros included).  Every sum runs in a fixed order (a segment's samples in increasing index, the
 * 4 n_orders time partials in index order, the segments from the last downwards): deterministic, no atomics, no workspace.
 * Device pointers in CSR order, asynchronous on the context's stream. */
int mrs_tg_plan_sample_states_vjp(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev, double sampling_dt,
                                  int32_t sample_capacity, int32_t n_orders, const double* grad_states_dev,
                                  const int32_t* status_dev, double* grad_coeffs_out_dev, double* grad_seg_times_out_dev,
                                  int32_t* sample_segment_out_dev, double* sample_time_out_dev, int32_t* n_samples_out_dev);

/* The state of every path at caller-given times (MRS_TG_CAP_EVALUATE; evaluate_kernel):
 * Trajectory::evaluate (trajectory.cpp:55-87) and what sampleTrajectoryAtTime / sampleFlatStateAtTime build on it.
 * query_times_dev [n_paths][n_queries], seconds from the start of that path's trajectory, in the caller's path order; any
 * order, duplicates allowed; a caller who wants fewer queries on some path pads with NaN.  The query t is located as the
 * reference does: acc = 0; for i = 0 .. S-1: acc += T_i, stop at the first i with acc > t (a query on a vertex belongs to
 * the segment on its right, zero-length segments are skipped); when no i stops the loop, i = S-1 (t equals the total);
 * start = acc - T_i, computed like that, and tau = t - start.  states_out_dev [n_paths][n_queries][n_orders][4] holds the
 * derivative orders 0 .. n_orders-1 (n_orders = 1 or MRS_TG_STATE_ORDERS) of (x, y, z, heading) at tau, evaluated as the
 * sampler evaluates (Horner over j!/(j-o)! c_j, the heading of order 0 wrapped to (-pi, pi]).  OUT OF RANGE -- t < 0,
 * t above the total, t not a number, or a total that is not a number -- gives a zero state row, segment -1 and local time 0
 * (the reference logs and returns a zero vector; here the segment index reports it).  query_segment_out_dev (index within
 * the path) and query_local_time_out_dev (tau), both [n_paths][n_queries], may be NULL.  n_queries == 0 succeeds and
 * touches nothing; n_queries is not bounded by the device's LDS, the segment count is (a plan whose longest path needs
 * more than 160 KB is refused).  Device pointers (16-byte aligned, as every allocator gives them) in CSR order,
 * asynchronous on the context's stream. */
int mrs_tg_plan_evaluate(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev, const double* query_times_dev,
                         int32_t n_queries, int32_t n_orders, double* states_out_dev, int32_t* query_segment_out_dev,
                         double* query_local_time_out_dev);
/* Backward pass of mrs_tg_plan_evaluate (evaluate_vjp_kernel): given the gradient of a loss L with
 * respect to the states, grad_states_dev [n_paths][n_queries][n_orders][4], writes dL/dcoeffs (grad_coeffs_out_dev
 * [sum S][4][10]), dL/dseg_times (grad_seg_times_out_dev [sum S]) and dL/dquery_times (grad_query_times_out_dev
 * [n_paths][n_queries]); at least one must be given.  An in-range query q in segment i at tau contributes
 *   dL/dc[i][dim][j] += sum_{o <= min(j, n_orders-1)} G[q][o][dim] j!/(j-o)! tau^(j-o)
 *   g_q               = sum_{o, dim} G[q][o][dim] p_dim^(o+1)(tau)       (order 4 takes the fifth derivative)
 *   dL/dt_q           = g_q,        dL/dT_m -= g_q for every segment m < i.
 * What is not smooth, and what the call does there:
 *   segment membership -- held fixed; a query on a vertex gets the right-hand segment's one-sided gradient, a query at
 *     the total time the last segment's;
 *   the floating-point start -- differentiated as the exact prefix: dtau/dT_m = -1 for m < i, 0 otherwise, dtau/dt = 1;
 *   heading wrap -- derivative 1;
 *   an out-of-range query -- contributes nothing and gets dL/dt = 0; its upstream row is never read (NaN there is harmless);
 *   with status_dev, a path with status <= 0 gets zero rows in all three outputs, whatever its coefficients hold;
 *   a segment without a query gets zero coefficient rows and still its time gradient from the queries behind it;
 *   a zero upstream entry contributes exactly 0.
 * Every output element that belongs to the plan is written exactly once (zeros included; with n_queries == 0 the
 * coefficient and time gradients are zeros).  Every sum runs in a fixed order -- a segment's queries in increasing query
 * index from 0.0, the 4 n_orders partials of g_q in the order o * 4 + dim, the segments from the last downwards --
 * whatever the order of the queries: deterministic, no atomics, no workspace, the same bits for a path wherever it sits in a
 * batch.  Device pointers in CSR order, asynchronous on the context's stream. */
int mrs_tg_plan_evaluate_vjp(mrs_tg_plan* plan, const double* coeffs_dev, const double* seg_times_dev,
                             const double* query_times_dev, int32_t n_queries, int32_t n_orders, const double* grad_states_dev,
                             const int32_t* status_dev, double* grad_coeffs_out_dev, double* grad_seg_times_out_dev,
                             double* grad_query_times_out_dev);

/* How far the sampled trajectory strays from the waypoint polyline (MRS_TG_CAP_DEVIATION; path_deviation_kernel, DESIGN.md
 * section 11b): validateTrajectorySpatial (mrs_trajectory_generation.cpp:1401-1455), the figure
 * check_trajectory_deviation/max_deviation acts on, as a plan step on samples where they are.
 * samples_dev [n_paths][sample_capacity][4] and n_samples_dev [n_paths] are what a solve or mrs_tg_plan_sample left
 * (n = min(n_samples, sample_capacity) rows are read, x, y, z of each); waypoints_dev [sum V][4] are the plan's S + 1
 * vertices per path (x, y, z read), both in the caller's path order.  With D = distFromSegment (:1533-1554) and the
 * cursor c_0 = 0, for the samples i = 0 .. n-2 of a path:
 *   d_i = D(s_i, w_c, w_{c+1}),  e_i = D(w_{c+1}, s_i, s_{i+1}),  c_{i+1} = c_i + 1 if e_i < 0.05 and c_i < S - 1, else c_i.
 * Sample i is COUNTED if c_i > 0, or first_segment != 0 (max_deviation_first_segment), or S + 1 <= 2.
 * Outputs, each may be NULL, at least one given:
 *   deviation_out_dev [n_paths][sample_capacity]  d_i of every scanned sample, counted or not; 0 in the rows >= n - 1
 *   cursor_out_dev [n_paths][sample_capacity]     c_i; -1 in the rows >= n - 1
 *   max_deviation_out_dev [n_paths]               the maximum over the counted samples (0 without any): the reference's
 *   argmax_out_dev [n_paths]                      the first counted sample whose d exceeded, strictly, every one in front
 *                                                 of it -- the reference's running maximum, which starts at 0: -1 when no
 *                                                 counted sample has d > 0
 *   segment_max_out_dev [sum S]                   the maximum over the counted samples whose cursor is that segment (0
 *                                                 without any): the reference's segment_safe is segment_max <= max_deviation
 * With status_dev, a path with status <= 0 gets zeros and cursor -1; a path with n <= 1 scans nothing.  A deviation that is
 * not a number never becomes a maximum (the reference's `>`).  The distance is devq::dist (csrc/mrs_tg_deviation.hpp), no
 * fused multiply-add, the function mrs_tg_optimize_paths' own scan (devq::validate) calls: the same bits.  Every output element that belongs to the plan is
 * written exactly once.  Device pointers (16-byte aligned), asynchronous on the context's stream. */
int mrs_tg_plan_path_deviation(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                               int32_t sample_capacity, const double* waypoints_dev, int32_t first_segment,
                               const int32_t* status_dev, double* deviation_out_dev, int32_t* cursor_out_dev,
                               double* max_deviation_out_dev, int32_t* argmax_out_dev, double* segment_max_out_dev);
/* Backward pass of mrs_tg_plan_path_deviation (path_deviation_vjp_kernel): given
 * grad_deviation_dev [n_paths][sample_capacity] = dL/dd_i (the rows >= n - 1 are never read), writes dL/dsamples
 * (grad_samples_out_dev [n_paths][sample_capacity][4]) and dL/dwaypoints (grad_waypoints_out_dev [sum V][4]); column 3 of
 * both is zero; at least one must be given.  The cursors are recomputed as the forward computes them.  With p = s_i,
 * a = w_c, b = w_{c+1}, d = d_i, and coord, len, the perpendicular component e as distFromSegment forms them:
 *   coord < 0     dd/dp = (p - a)/d,  dd/da = -dd/dp,        dd/db = 0
 *   coord > len   dd/dp = (p - b)/d,  dd/da = 0,             dd/db = -dd/dp
 *   otherwise     dd/dp = u = e/d,    dd/da = -(1 - tau) u,  dd/db = -tau u,   tau = coord/len
 * What is not smooth, and what the call does there:
 *   the cursor -- held fixed: the advance test e_i < 0.05 is piecewise constant, nothing flows through s_{i+1};
 *   the branch -- the forward's; coord == 0 and coord == len take the interior row (its one-sided gradient);
 *   coincident waypoints (len == 0) -- the interior row with tau = 0: everything goes to a;
 *   a sample on its segment (d == 0) -- contributes exactly 0;
 *   a zero upstream entry contributes exactly 0;
 *   with status_dev, a path with status <= 0 gets zero rows in both outputs.
 * Every sum runs in a fixed order: a waypoint's accumulator starts at 0.0 and takes, in increasing sample index, the
 * b-parts of the samples whose cursor is the segment in front of it, then the a-parts of the samples whose cursor is its
 * own segment.  Deterministic, no atomics, no workspace, the same bits for a path wherever it sits in a batch; every output
 * element that belongs to the plan is written exactly once.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_path_deviation_vjp(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                   int32_t sample_capacity, const double* waypoints_dev, const int32_t* status_dev,
                                   const double* grad_deviation_dev, double* grad_samples_out_dev,
                                   double* grad_waypoints_out_dev);

/* The Euclidean segment-time estimate as a plan step (MRS_TG_CAP_ESTIMATE_GRADIENT; estimate_times_kernel, DESIGN.md section
 * 4e): estimateSegmentTimesEuclidean (vertex.cpp:491-565), the times a solve with options.estimate_times = 1 starts from,
 * without a solve.  waypoints_dev [sum V][4] are the plan's S + 1 vertices per path (x, y, z, unwrapped heading), limits_dev
 * [n_paths][9] (index 3 (k - 1) + group; entries 0, 1, 2 and 5 are read), both in the caller's path order;
 * seg_times_out_dev [sum S].  The kernel is the solve's own: the result is, bit for bit, what mrs_tg_plan_solve with
 * estimate_times = 1 and MRS_TG_TIME_ALLOC_NONE leaves in seg_times_inout.  Device pointers, asynchronous on the context's
 * stream. */
int mrs_tg_plan_estimate_times(mrs_tg_plan* plan, const double* waypoints_dev, const double* limits_dev,
                               double* seg_times_out_dev);
/* Backward pass of mrs_tg_plan_estimate_times (estimate_times_vjp_kernel): given grad_seg_times_dev
 * [sum S] = dL/dt_i, writes dL/dwaypoints (grad_waypoints_out_dev [sum V][4]), dL/dlimits (grad_limits_out_dev [n_paths][9])
 * and the term every segment's time came from (term_out_dev [sum S], MRS_TG_ESTIMATE_TERM_*).  At least one of the three
 * must be given; the two gradients need grad_seg_times_dev, term_out_dev alone does not.  The term is decided by the
 * forward's own expressions in the forward's order.  With G = dL/dt_i, start s, end e, d = e - s, h = sqrt(dx^2 + dy^2),
 * delta the forward's signed wrapped heading difference (start minus end), ang = |delta|, w = limits[2], a = limits[5]:
 *   HORIZONTAL  dt/de = (dx/h, dy/h, 0, 0)/v_h          dt/dv_h = -(h/v_h)/v_h
 *   VERTICAL    dt/de = (0, 0, sign(dz), 0)/v_v         dt/dv_v = -(|dz|/v_v)/v_v
 *   FLOOR       0                                       0
 *   HEADING     dt/de = (0, 0, 0, -1.5 sign(delta)/w)   dt/dw = 1.5 (-ang/w^2 - [cruise] 1/a + [acc] 2/a)
 *                                                       dt/da = 1.5 ([cruise] w/a^2 - [acc] 2 w/a^2)
 * and dt/ds = -dt/de; cruise is the forward's `reduced >= 0` branch, acc is ang > pi/4.  No transcendental enters a
 * gradient's value.  What is not smooth, and what the call does there:
 *   every branch -- the regime, the floor, heading-wins, cruise / acc -- is the forward's and is held fixed;
 *   a tie between the heading term and the distance term stays with the distance term;
 *   equal headings (delta == 0) have sign 0; at the +-pi seam the gradient is the one-sided value;
 *   a relaxed heading (a heading limit >= FLT_MAX) never takes HEADING;
 *   coincident waypoints land on FLOOR, so h = 0 is never divided by; a purely vertical segment is VERTICAL;
 *   a zero upstream entry contributes exactly 0;
 *   a segment with a non-finite waypoint or time, or a limit that is not a number, contributes zeros and reports FLOOR.
 * Every sum runs in a fixed order: a vertex's accumulator starts at 0.0 and takes the end-part of the segment in front of
 * it, then the start-part of its own segment; a path's nine limit gradients start at 0.0 and take its segments in increasing
 * index; entries 3, 4, 6, 7 and 8 are always 0.  Deterministic, no atomics, no workspace, the same bits for a path wherever
 * it sits in a batch; every output element that belongs to the plan is written exactly once, zeros included.  Device
 * pointers, asynchronous on the context's stream. */
int mrs_tg_plan_estimate_times_vjp(mrs_tg_plan* plan, const double* waypoints_dev, const double* limits_dev,
                                   const double* grad_seg_times_dev, double* grad_waypoints_out_dev,
                                   double* grad_limits_out_dev, int32_t* term_out_dev);

/* Where the sampled trajectory passes the requested waypoints (MRS_TG_CAP_WAYPOINT_PASSAGE; waypoint_passage_kernel, DESIGN.md
 * section 11c): getWaypointInTrajectoryIdxs (mrs_trajectory_generation.cpp:1461-1499), the waypoint_trajectory_idxs of the
 * service's response, as a plan step on samples where they are -- with the miss distance and the place of the foot point on
 * the step, which say how closely and WHEN a waypoint is passed.
 * samples_dev [n_paths][sample_capacity][4] and n_samples_dev [n_paths] are what a solve or mrs_tg_plan_sample left
 * (n = min(n_samples, sample_capacity) rows are read, x, y, z of each).  The waypoints are the ones the caller asks about,
 * which need not be the plan's vertices: wp_offsets_dev [n_paths + 1] (int32, device memory, the caller's path order) is a
 * CSR over waypoints_dev [sum W][4] (x, y, z read), path p owning the rows wp_offsets[p] .. wp_offsets[p + 1] - 1 (W = 0 is
 * allowed; W has no upper bound).  wp_offsets_dev == NULL means the plan's own vertices: path p's rows start at
 * seg_offsets[p] + p and W = S + 1.  With D = distFromSegment (:1533-1554) and the cursor c = 0, for i = 0 .. n-2 of a path:
 *   m = D(w_c, s_i, s_{i+1});   if m < 0.1:  index[c] = i, miss[c] = m, fraction[c] = tau, c = c + 1;   stop when c == W
 * tau is the place of the foot point on the step s_i -> s_{i+1}, from the very coord and len that D forms: 0 when coord < 0
 * or len * len == 0, 1 when coord > len, otherwise coord / len.  The passing time of waypoint k is
 * (index[k] + fraction[k]) * sampling_dt.  A step takes at most one waypoint: the indices increase strictly.  A distance that
 * is not a number is no hit.  Outputs, each may be NULL, at least one given:
 *   index_out_dev [sum W] (int32)  the step at which waypoint k is passed; -1 for every waypoint from the first one not
 *                                  reached on, even if a later one lies near the trajectory (the reference never tests it)
 *   count_out_dev [n_paths]        how many were reached: the reference's idxs.size()
 *   miss_out_dev [sum W]           m of the hit; 0.0 where not reached
 *   fraction_out_dev [sum W]       tau of the hit; 0.0 where not reached
 * With status_dev, a path with status <= 0 gets count 0, indices -1 and zeros; n <= 1 or W = 0 scans nothing.  The hit
 * test is passq::hit (csrc/mrs_tg_passage.hpp: devq::dist, no fused multiply-add), which mrs_tg_waypoint_trajectory_idxs calls too:
 * index and count are its on the same samples.  Every output element that belongs to the plan is written exactly once, in the caller's path order.
 * Device pointers (16-byte aligned), asynchronous on the context's stream. */
int mrs_tg_plan_waypoint_passage(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                 int32_t sample_capacity, const int32_t* wp_offsets_dev, const double* waypoints_dev,
                                 const int32_t* status_dev, int32_t* index_out_dev, int32_t* count_out_dev,
                                 double* miss_out_dev, double* fraction_out_dev);
/* Backward pass of mrs_tg_plan_waypoint_passage (waypoint_passage_vjp_kernel): given grad_miss_dev
 * [sum W] = dL/dmiss and grad_fraction_dev [sum W] = dL/dfraction (either may be NULL, which counts as zero; entries of
 * waypoints that are not reached are never read), writes dL/dsamples (grad_samples_out_dev [n_paths][sample_capacity][4])
 * and dL/dwaypoints (grad_waypoints_out_dev [sum W][4]); column 3 of both is zero; at least one must be given.  The scan is
 * recomputed as the forward computes it.  For a hit of p = w_k on the step a = s_i, b = s_{i+1}: the miss part is the row of
 * mrs_tg_plan_path_deviation_vjp's table for D(p, a, b); the fraction part is zero in the two clamped branches and for
 * len * len == 0, and in the interior, with v = b - a, q = p - a, L2 = len * len:
 *   dtau/dp = v / L2,   dtau/db = (q - 2 tau v) / L2,   dtau/da = -dtau/dp - dtau/db
 * What is not smooth, and what the call does there:
 *   the index -- held fixed: the test m < 0.1 is piecewise constant;
 *   the branch -- the forward's; coord == 0 and coord == len take the interior row;
 *   a waypoint on its step (m == 0) -- contributes exactly 0 through the miss;
 *   a zero upstream contributes exactly 0;
 *   waypoints that are not reached, and with status_dev the paths with status <= 0, get zero rows.
 * Every sum runs in a fixed order: a hit's contribution to a row is, per coordinate, the miss part plus the fraction part;
 * a waypoint's row is that one term; sample row j starts at 0.0 and takes the b-contribution of the hit on step j - 1, if
 * there is one, then the a-contribution of the hit on step j, if there is one.  The rows from n on are zero.  Deterministic,
 * no atomics, no workspace, the same bits for a path wherever it sits in a batch; every output element that belongs to the
 * plan is written exactly once.  Device pointers (16-byte aligned), asynchronous on the context's stream. */
int mrs_tg_plan_waypoint_passage_vjp(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                     int32_t sample_capacity, const int32_t* wp_offsets_dev, const double* waypoints_dev,
                                     const int32_t* status_dev, const double* grad_miss_dev, const double* grad_fraction_dev,
                                     double* grad_samples_out_dev, double* grad_waypoints_out_dev);

/* The Baca segment-time estimate as a plan step (MRS_TG_CAP_BACA; baca_times_kernel):
 * estimateSegmentTimesBaca (vertex.cpp:301-485) -- the reference's yardstick for accepting a trajectory and the clock of its
 * fallback sampler -- for every path of the plan, where the waypoints are.  waypoints_dev [sum V][4] are the plan's S + 1
 * vertices per path (x, y, z, unwrapped heading), limits_dev [n_paths][9] (index 3 (k - 1) + group; entries 0 .. 7 are read,
 * entry 8 is not), both in the caller's path order; seg_times_out_dev [sum S].  One lane per segment.  A segment's neighbours
 * are the neighbours inside its own path: segment 0 takes the full acceleration time in front, segment S - 1 behind, S = 1
 * both.  The arithmetic is the host estimate's, operation by operation, without fused multiply-adds, but the result is NOT
 * promised in the host's bits: atan2, sin and cos are the device's (the estimate is continuous across its inclination
 * branches, so their last bit moves the value by roundings only; 1e-13 relative).  mrs_tg_estimate_times_baca,
 * mrs_tg_find_trajectory and mrs_tg_optimize_paths keep their host arithmetic.  Device pointers, asynchronous on the
 * context's stream. */
int mrs_tg_plan_estimate_times_baca(mrs_tg_plan* plan, const double* waypoints_dev, const double* limits_dev,
                                    double* seg_times_out_dev);
/* Backward pass of mrs_tg_plan_estimate_times_baca (baca_times_vjp_kernel): given grad_seg_times_dev
 * [sum S] = dL/dt_i, writes dL/dwaypoints (grad_waypoints_out_dev [sum V][4]), dL/dlimits (grad_limits_out_dev [n_paths][9])
 * and the branches every segment's time took (flags_out_dev [sum S], bits MRS_TG_BACA_*).  At least one of the three must be
 * given; the two gradients need grad_seg_times_dev, flags_out_dev alone does not.  Every branch is decided by the forward's
 * own calls in the forward's order and is held fixed.  With G = dL/dt_i, pre, s, e, post the four waypoints a segment reads,
 * d = e - s, D = |d|, h = sqrt(dx^2 + dy^2), and for L in {v, a, j}: c_L = L_h, q_L = h (horizontal regime) or c_L = L_v,
 * q_L = |dz| (vertical regime), grad q = (dx/h, dy/h, 0) or (0, 0, sign dz), rho_L = grad q_L / q_L:
 *   L_max = c_L D / q_L                    (the forward's |L_h / cos| or |L_v / sin| up to roundings)
 *   full  = v_max/a_max + a_max/j_max      dfull/de = (v_max/a_max)(rho_a - rho_v) + (a_max/j_max)(rho_j - rho_a)
 *   cap   = sqrt(2 D / a_max)              dcap/de = cap rho_a / 2               dcap/dc_a = -(cap/2)/c_a
 *   u1 = (s - pre)/n1, u2 = d/D, u3 = (post - e)/n3, dot1 = u1.u2, dot2 = u2.u3    (the forward's unit vectors)
 *   c1 = 1 (segment 0, or DOT1_CLAMPED), else 1 - dot1;   c2 = 1 (segment S - 1, or DOT2_CLAMPED), else 1 - dot2
 *   t = D/v_max + t1 + t2,   t_i = c_i full, or cap where T_i_CAPPED
 *   D/v_max = q_v/c_v   d/de = grad q_v / c_v                         d/dc_v = -(q_v/c_v)/c_v
 *   t_i = c_i full      d/de = c_i dfull/de + full dc_i/de            d/dc_v = c_i (v_max/a_max)/c_v
 *                       d/dc_a = -c_i (v_max/a_max)/c_a + c_i (a_max/j_max)/c_a     d/dc_j = -c_i (a_max/j_max)/c_j
 *   c1 = 1 - dot1       dc1/dpre = (u2 - dot1 u1)/n1   dc1/ds = -(u2 - dot1 u1)/n1 + (u1 - dot1 u2)/D   dc1/de = -(u1 - dot1 u2)/D
 *   c2 = 1 - dot2       dc2/ds = (u3 - dot2 u2)/D      dc2/de = -(u3 - dot2 u2)/D + (u2 - dot2 u3)/n3   dc2/dpost = -(u2 - dot2 u3)/n3
 *   d/ds = -d/de for D/v_max, full and cap
 *   FLOOR    0
 *   HEADING  dt/de = (0, 0, 0, -1.5 sign(delta)/w), dt/ds its negative;  dt/dw = 1.5 (-ang/w^2 - [cruise] 2/a + [acc] 2/a)
 *            dt/da = 1.5 ([cruise] 2 w/a^2 - [acc] 2 w/a^2)
 * with delta the forward's signed wrapped heading difference (start minus end), ang = |delta|, w = limits[2], a = limits[5]:
 * the heading row of mrs_tg_plan_estimate_times_vjp, with this estimator's `2 *` in front of w^2/a in the cruise branch.  No
 * transcendental enters a gradient's value.  What is not smooth, and what the call does there:
 *   ties stay with the forward's comparison, all strict: t_i > cap, dot < 0, the heading term > t, t < 0.01;
 *   a zero-length neighbour has the zero unit vector as in the forward, and gives no gradient through it;
 *   FLOOR gives zeros; HEADING gives the heading row only; a relaxed heading (a heading limit >= FLT_MAX) never takes HEADING;
 *   a zero upstream entry contributes exactly 0;
 *   a segment that reads a non-finite waypoint or limit, or whose time is not finite, contributes zero rows and has flags = FLOOR;
 *   limit entry 8 is always 0.
 * Every sum runs in a fixed order: a segment's part is the sum from 0.0 of its addends in the order above (D/v_max, t1, t2),
 * times G; a vertex's accumulator starts at 0.0 and takes, of the segments that exist, the post-part of segment v - 2, the
 * end-part of v - 1, the start-part of v, the pre-part of v + 1 (increasing segment index); a path's nine limit gradients start
 * at 0.0 and take its segments in increasing index.  Deterministic, no atomics, no workspace, the same bits for a path wherever
 * it sits in a batch; every output element that belongs to the plan is written exactly once, zeros included.  Device pointers,
 * asynchronous on the context's stream. */
int mrs_tg_plan_estimate_times_baca_vjp(mrs_tg_plan* plan, const double* waypoints_dev, const double* limits_dev,
                                        const double* grad_seg_times_dev, double* grad_waypoints_out_dev,
                                        double* grad_limits_out_dev, int32_t* flags_out_dev);
/* The nodelet's gate on a finished trajectory as a plan step (length_gate_kernel): per path the total of
 * seg_times_dev [sum S] (from 0.0, in increasing index: initial_total_time_baca when the times are the Baca estimate's) into
 * total_out_dev [n_paths], and into verdict_out_dev [n_paths] one of MRS_TG_FIND_*: REJECTED_CODE first, when status_dev
 * [n_paths] is given and the code is one the nodelet rejects (accepted: >= 1 except 6, and -1); then, with len =
 * (double)n_samples_dev[p] * sampling_dt (the raw count a solve leaves), REJECTED_TOO_LONG when len > max_factor * total,
 * REJECTED_TOO_SHORT when len < min_factor * total, else ACCEPTED.  A trajectory that is not longer than one second passes
 * (!(len > 1.0)); a factor <= 0 switches its side off.  No fused multiply-add: with the same seg_times the total and the
 * verdict are mrs_tg_find_trajectory's, bit for bit.  The step has no capacity argument: a count of sample_capacity + 1 (the
 * sampler's overflow report, a LOWER bound of the real count) must not be handed to it as it is -- it can come back as
 * REJECTED_TOO_SHORT; the caller refuses n_samples > sample_capacity itself, as mrs_tg_optimize_paths does, or switches the
 * lower side off for such a path, as mrs_tg_find_trajectory does.  status_dev may be NULL; either output may be NULL, not
 * both.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_length_gate(mrs_tg_plan* plan, const double* seg_times_dev, const int32_t* n_samples_dev, double sampling_dt,
                            double max_factor, double min_factor, const int32_t* status_dev, double* total_out_dev,
                            int32_t* verdict_out_dev);

/* The heading unwrap as a plan step (MRS_TG_CAP_FALLBACK_SAMPLE; unwrap_headings_kernel): the
 * sequential sradians::unwrap of findTrajectory / findTrajectoryFallback (:1233-1241) for every path of the plan.  waypoints_dev
 * [sum V][4]; in waypoints_out_dev [sum V][4] vertex v of a path carries its heading unwrapped against the UNWRAPPED heading of
 * vertex v - 1 (vertex 0 against itself), x, y, z copied.  One lane per path.  fmod, additions and comparisons only: the host's
 * bits.  waypoints_out_dev == waypoints_dev is allowed; any other overlap is not.  What mrs_tg_plan_estimate_times_baca wants
 * for its fourth column.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_unwrap_headings(mrs_tg_plan* plan, const double* waypoints_dev, double* waypoints_out_dev);
/* The fallback sampler as a plan step (fallback_sample_kernel): the interpolation loop of
 * findTrajectoryFallback (:1327-1381) -- what a request gets that asks for it or runs over its time budget -- for every path of
 * the plan: constant-rate interpolation of the waypoint polyline on seg_times_dev [sum S] (the reference: the Baca estimate of
 * the unwrapped waypoints under the fallback's limits, mrs_tg_plan_estimate_times_baca).  waypoints_dev [sum V][4] are the RAW
 * waypoints (x, y, z, heading as requested: :1362 interpolates those), stop_at_dev [sum V] (may be NULL: nobody stops; a path's
 * first entry is ignored, its last never read) says where the trajectory dwells.  With insert = (int)round(stopping_time /
 * sampling_dt), segment i of a path of S segments with time t gives
 *   nd = (t > 0.1) ? ceil(t / sampling_dt) : 0          (strictly; a NaN or negative time: 0)
 *   rows = nd + (nd > 0 && i == S - 1) + ((nd > 0 && i > 0 && stop_at[i]) ? insert : 0)
 * and its row r (0-based) is, with j = max(r - inserted rows, 0) and coeff = (double)j * (1.0 / nd),
 *   a + coeff (b - a) for x, y, z (no fused multiply-add: the host's bits) and
 *   wrap_yaw(radians::interp(a_heading, b_heading, coeff)), the quaternion round trip setFromYaw / getYaw (sin, cos and atan2
 *   are the device's: the heading is the host's up to their roundings, a last-bit flip between -pi and pi included).
 * samples_out_dev [n_paths][sample_capacity][4]; n_samples_out_dev [n_paths] follows the solve's convention: the count when it
 * fits, sample_capacity + 1 when it does not, and rows from min(count, sample_capacity) on are NOT written.
 * seg_first_row_out_dev [sum S] (may be NULL): the row at which a segment's samples start, saturated at sample_capacity + 1; a
 * segment without rows reports the row at which the next one starts.  A path none of whose segments is longer than 0.1 s has
 * no rows; one whose last segment has none does not reach its last waypoint (the reference's behaviour).  Counts are 64-bit
 * sums; a time of +inf takes part with a count of 2^31.  One wavefront per path.  MRS_TG_ERR_INVALID_ARG, before any launch:
 * sampling_dt not positive and finite, stopping_time negative or not finite, an insert that does not fit int32,
 * sample_capacity < 1 or > INT32_MAX - 1, a missing mandatory pointer.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_fallback_sample(mrs_tg_plan* plan, const double* waypoints_dev, const uint8_t* stop_at_dev,
                                const double* seg_times_dev, double sampling_dt, double stopping_time, int32_t sample_capacity,
                                int32_t* n_samples_out_dev, double* samples_out_dev, int32_t* seg_first_row_out_dev);
/* Backward pass of mrs_tg_plan_fallback_sample (fallback_sample_vjp_kernel): given grad_samples_dev
 * [n_paths][sample_capacity][4] = dL/dsamples, writes dL/dwaypoints (grad_waypoints_out_dev [sum V][4]).  The counts are the
 * forward's (the same device function on the same stop_at_dev, seg_times_dev, sampling_dt and stopping_time) and are held fixed:
 * seg_times receives no gradient.  Row r of segment i gives vertex i the weight 1.0 - coeff and vertex i + 1 the weight coeff,
 * all four columns alike: the heading column is the almost-everywhere derivative of wrap_yaw o radians::interp, its wrap seams
 * and the direction chosen at a heading difference of exactly +-pi held fixed.  Every sum runs in a fixed order: vertex v's row
 * starts at 0.0, takes the rows of segment v - 1 in increasing row index, each addend coeff * g rounded and then added, then the
 * rows of segment v in increasing row index, each addend (1.0 - coeff) * g.  Only rows below min(count, sample_capacity) are
 * read.  Deterministic, no atomics, no workspace, the same bits for a path wherever it sits in a batch; every element of
 * grad_waypoints_out_dev that belongs to the plan is written exactly once, zeros included.  The argument checks are the
 * forward's.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_fallback_sample_vjp(mrs_tg_plan* plan, const uint8_t* stop_at_dev, const double* seg_times_dev, double sampling_dt,
                                    double stopping_time, int32_t sample_capacity, const double* grad_samples_dev,
                                    double* grad_waypoints_out_dev);

/* Path thinning as a plan step (MRS_TG_CAP_PATH_EDIT; thin_path_kernel, vertex_offsets_kernel, edit_write_kernel; DESIGN.md
 * section 11e): preprocessPath (:431-500) for every path of the plan, where the waypoints are.  The plan is the plan of the INPUT
 * paths: waypoints_dev [sum V][4] are its S + 1 vertices per path with their RAW headings, stop_at_dev [sum V] may be NULL
 * (nobody stops).  Vertex i of a path of n vertices is kept behind the last kept vertex `last` as the reference's loop decides:
 * the first and the last vertex always; an interior one is dropped when the straightener is enabled, n >= 3 and every vertex j
 * in (last, i] stays within straightener_max_deviation of the segment wp[last] -> wp[i + 1] and passes both SIGNED heading
 * comparisons (quirk B3 of the reference: radians::diff(first, mid) > limit, radians::diff(last, mid) > limit, no absolute value),
 * else when sqrt(dx^2 + dy^2 + dz^2) < min_waypoint_distance against wp[last].  Comparisons as the host writes them: a NaN
 * compares false everywhere.  No fused multiply-add, sqrt and fmod only: the rows mrs_tg_optimize_paths keeps, bit for bit.
 * The result is PACKED, the batch a new plan can be created on: vertex_offsets_out_dev [n_paths + 1] (the first vertex of every
 * edited path in the caller's path order, the total behind them), waypoints_out_dev [sum V][4] and, each NULL or written,
 * stop_at_out_dev [sum V] and source_out_dev [sum V]: the batch-wide index of the input vertex an output vertex copies.  Every
 * element below vertex_offsets_out[n_paths] is written exactly once, nothing at or behind it.  The caller reads
 * vertex_offsets_out back (n_paths + 1 integers) to create the next plan: mrs_tg_plan_create takes host offsets.  The outputs may
 * not overlap the inputs.  Three launches on the context's stream (one wavefront per path decides and counts, ONE workgroup sums
 * the counts, one lane per output vertex writes); no kernel waits for another workgroup, no atomics.  MRS_TG_ERR_INVALID_ARG,
 * before any launch: a missing mandatory pointer; a negative or NaN min_waypoint_distance or straightener threshold; sum V beyond
 * int32.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_preprocess_path(mrs_tg_plan* plan, const double* waypoints_dev, const uint8_t* stop_at_dev,
                                double min_waypoint_distance, int32_t straightener_enabled, double straightener_max_deviation,
                                double straightener_max_hdg_deviation, int32_t* vertex_offsets_out_dev, double* waypoints_out_dev,
                                uint8_t* stop_at_out_dev, int32_t* source_out_dev);
/* Mid-point subdivision as a plan step (insert_midpoints_kernel, vertex_offsets_kernel, edit_write_kernel; DESIGN.md section
 * 11e): :739-753 of optimize() for every path of the plan.  segment_max_dev [sum S] is mrs_tg_plan_path_deviation's
 * segment_max_out; a segment is unsafe when segment_max > max_deviation (the reference's d_seg > max_deviation on the maxima the
 * deviation step reports; a NaN is never unsafe).  Original segment s of a path of V vertices gets the mid-point
 * interpolatePoint(a, b, 0.5) (a + 0.5 (b - a) for x, y, z without a fused multiply-add, radians::interp for the raw heading: the
 * host's bits) when it is unsafe AND (s > 0 OR first_segment OR V <= 2), V counted before any insertion.  A path with
 * active_dev[p] == 0 (active_dev [n_paths], NULL = all) is copied unchanged: finished or failed paths.  The result is packed as
 * mrs_tg_plan_preprocess_path packs it: vertex_offsets_out_dev [n_paths + 1], waypoints_out_dev [sum V + sum S][4] and, each
 * NULL or written, stop_at_out_dev (0 for a mid-point), source_out_dev (for a mid-point the first vertex of its segment) and
 * inserted_out_dev (1 for a mid-point).  A subdivided path may exceed MRS_TG_MAX_SEGMENTS: the step reports it, and
 * mrs_tg_plan_create refuses it.  MRS_TG_ERR_INVALID_ARG, before any launch: a missing mandatory pointer; a negative or NaN
 * max_deviation; sum V + sum S beyond int32.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_insert_midpoints(mrs_tg_plan* plan, const double* waypoints_dev, const uint8_t* stop_at_dev,
                                 const double* segment_max_dev, double max_deviation, int32_t first_segment,
                                 const uint8_t* active_dev, int32_t* vertex_offsets_out_dev, double* waypoints_out_dev,
                                 uint8_t* stop_at_out_dev, int32_t* source_out_dev, uint8_t* inserted_out_dev);
/* Backward pass of both edit steps (path_edit_vjp_kernel): given vertex_offsets_dev, source_dev and
 * inserted_dev as the step wrote them (inserted_dev NULL after thinning) and grad_waypoints_edited_dev [sum V'][4] = dL/d(edited
 * waypoints), writes dL/dwaypoints (grad_waypoints_out_dev [sum V][4]) of the plan's INPUT vertices.  Nothing is recomputed: one
 * lane per input vertex finds its copies in its path's run of source_dev, which is non-decreasing, by binary search.  Vertex v's
 * row starts at 0.0 and takes, in this order, 0.5 * g (rounded, then added) of the mid-point of the segment in front of it, g of
 * its own copy, 0.5 * g of the mid-point of its own segment.  All four columns alike: the heading column is the almost-everywhere
 * derivative of radians::interp, its wrap held fixed.  A dropped vertex gets a zero row.  Deterministic, no atomics; every element
 * that belongs to the plan is written exactly once.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_path_edit_vjp(mrs_tg_plan* plan, const int32_t* vertex_offsets_dev, const int32_t* source_dev,
                              const uint8_t* inserted_dev, const double* grad_waypoints_edited_dev, double* grad_waypoints_out_dev);

/* The heading along the direction of travel as a plan step (MRS_TG_CAP_TRAVEL_HEADING; travel_heading_kernel, DESIGN.md section
 * 11f): getTrajectoryReference with override_heading_atan2 (mrs_trajectory_generation.cpp:1578-1603) for every path of the plan,
 * on samples where they are.  samples_dev [n_paths][sample_capacity][4] and n_samples_dev [n_paths] are what a solve, a sampler or
 * the fallback sampler left; n = min(n_samples, sample_capacity) rows count (a count of sample_capacity + 1 is sample_capacity
 * rows).  For the rows i = 0 .. n-2, with (dx, dy) = (x, y)_{i+1} - (x, y)_i and dist = sqrt(dx dx + dy dy) (written out, no
 * hypot, no fused multiply-add: csrc/mrs_tg_heading.hpp),
 *   heading_i = heading_{i-1}  if dist < min_step and i > 0,   else atan2(dy, dx)   (row i is then a SOURCE).
 * Row 0 is always a source (a zero step gives 0); a distance that is not a number makes a source with a heading that is not a
 * number, which the slow rows behind it carry.  Row n-1 keeps its heading; n <= 1 changes nothing; rows from n on are not
 * written; with status_dev (may be NULL) a path with status <= 0 is not touched.  A carried row holds exactly the bits of its
 * source's heading: a copy, not a second atan2.  atan2 is the device's: a source's heading is the host's up to its rounding.
 * The reference decides on std::hypot; the written-out distance is within an ulp of it, so the decision can differ from
 * mrs_tg_optimize_paths' host loop only for a step within an ulp of min_step.
 * samples_out_dev may be samples_dev: then only the heading of the rows 0 .. n-2 is stored.  Otherwise the rows 0 .. n-1 are
 * written whole, x, y, z (and the heading of row n-1) copied bit for bit, and the two arrays may not overlap.  source_out_dev
 * [n_paths][sample_capacity] (may be NULL): the row whose step gave this row's heading, -1 for row n-1, not written from n on.
 * One wavefront per path; no LDS, no atomics, no workspace; the plan contributes its path count and its context.
 * MRS_TG_ERR_INVALID_ARG, before any launch: a negative sample_capacity, a missing mandatory pointer, a min_step that is not
 * finite (0.05 is the reference's).  Device pointers (16-byte aligned), asynchronous on the context's stream. */
int mrs_tg_plan_travel_heading(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev, int32_t sample_capacity,
                               const int32_t* status_dev, double min_step, double* samples_out_dev, int32_t* source_out_dev);
/* Backward pass of mrs_tg_plan_travel_heading (travel_heading_vjp_kernel): given grad_out_dev
 * [n_paths][sample_capacity][4] = dL/d(output rows), writes dL/dsamples (grad_samples_out_dev [n_paths][sample_capacity][4]) of
 * the INPUT rows samples_dev.  The sources are recomputed as the forward computes them and held fixed.  x, y, z of the upstream
 * pass through; row n-1 passes its heading entry through; every other heading entry is 0 (the input headings of the rows
 * 0 .. n-2 are not read by the forward).  A source s collects G_s, the sum of grad_out[i][3] over the rows i of its run -- from s
 * up to but excluding the next source, at most row n-2 -- from 0.0 in increasing i; with r2 = dx dx + dy dy of its step it adds
 *   (+dy / r2 * G_s, -dx / r2 * G_s) to x, y of row s   and   (-dy / r2 * G_s, +dx / r2 * G_s) to x, y of row s + 1,
 * both exactly 0 when r2 == 0.  The terms of a row's x (and y) are added in this order: the upstream, the term of the row's own
 * step, the term of the step of the row in front.  Rows from n on are zero; with status_dev, a path with status <= 0 gets zero
 * rows.  Deterministic, no atomics, no workspace, the same bits on every call and for a path wherever it sits in a batch; every
 * element that belongs to the plan is written exactly once.  grad_out_dev and grad_samples_out_dev may not overlap.  The
 * argument checks are the forward's.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_travel_heading_vjp(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                   int32_t sample_capacity, const int32_t* status_dev, double min_step, const double* grad_out_dev,
                                   double* grad_samples_out_dev);

/* Where a trajectory starts, as a plan step (MRS_TG_CAP_INITIAL_CONDITION; initial_condition_kernel, csrc/mrs_tg_initial.hpp,
 * DESIGN.md section 11g): prepareInitialCondition (mrs_trajectory_generation.cpp:506-614) and the first-waypoint rule
 * (:650-655) for every path of the plan, one lane per path; the batched form of mrs_tg_prepare_initial_condition, the same
 * table and the same bins.  The plan contributes its path count and its context only (mrs_tg_plan_create refuses a path without
 * a segment, and a request of one waypoint is the normal case here): the requested waypoints are addressed by
 * vertex_offsets_dev [n_paths + 1], of which this call reads the counts for the n_path_waypoints >= 2 rule; a path may have no
 * vertex or one.  Inputs, [n_paths] each:
 *   flags_dev                 bit 0 a tracker command is present, bit 1 a UAV state is present, bit 2 dont_prepend
 *   tracker_dev [.][4][4]     row 0 the pose x, y, z, heading, rows 1 .. 3 velocity, acceleration, jerk (xyz + the heading's)
 *   tracker_age_dev           now - its stamp (> 1.0: stale);   uav_pose_dev [.][4]  x, y, z, heading
 *   path_time_offset_dev      path stamp - now (0 for an unstamped path)
 *   pred_*_dev [.][pred_capacity][4], n_pred_dev   the prediction in mrs_tg_prediction's layout, n_pred rows of it valid
 *                             (pred_capacity 0: the arrays may be NULL)
 * takeoff_height is one scalar.  Outputs: decision_out_dev (MRS_TG_IC_*), sample_offset_out_dev (k, as
 * mrs_tg_prepare_initial_condition reports it: set when the tracker command is used for an offset > 0.2 s, else 0) and
 * initial_out_dev [.][4][4]: row 0 the prepended waypoint, whose heading is also the state's heading, rows 1 .. 3 the
 * derivatives; the whole block is zero where MRS_TG_IC_PREPEND is not set.  Every value is a copy of an input but
 * z + takeoff_height.  k and the 0.2 s threshold are evaluated in double, in the host's order, the quotient by a division.
 * MRS_TG_ERR_INVALID_ARG, before any launch: a missing pointer (all are mandatory), a negative pred_capacity, a NaN
 * takeoff_height.  Device pointers (16-byte aligned), asynchronous on the context's stream. */
int mrs_tg_plan_initial_condition(mrs_tg_plan* plan, const int32_t* flags_dev, const double* tracker_dev,
                                  const double* tracker_age_dev, const double* uav_pose_dev, double takeoff_height,
                                  const double* path_time_offset_dev, const int32_t* vertex_offsets_dev,
                                  const double* pred_position_dev, const double* pred_velocity_dev,
                                  const double* pred_acceleration_dev, const double* pred_jerk_dev, const int32_t* n_pred_dev,
                                  int32_t pred_capacity, int32_t* decision_out_dev, int32_t* sample_offset_out_dev,
                                  double* initial_out_dev);
/* Backward pass of mrs_tg_plan_initial_condition (initial_condition_vjp_kernel), the decision and k held fixed: given
 * grad_initial_dev [n_paths][4][4] writes grad_tracker_out_dev [n_paths][4][4] (the block where FROM_TRACKER is set),
 * grad_uav_out_dev [n_paths][4] (row 0 of the block where FROM_UAV is set) and the four grad_pred_*_out_dev
 * [n_paths][pred_capacity][4], where row k of each carries row 0 .. 3 of the block where FROM_PREDICTION is set.  Every
 * other element is zero.  Copies only; every element of every output is written exactly once; the same bits on every call. */
int mrs_tg_plan_initial_condition_vjp(mrs_tg_plan* plan, const int32_t* decision_dev, const int32_t* sample_offset_dev,
                                      const double* grad_initial_dev, int32_t pred_capacity, double* grad_tracker_out_dev,
                                      double* grad_uav_out_dev, double* grad_pred_position_out_dev,
                                      double* grad_pred_velocity_out_dev, double* grad_pred_acceleration_out_dev,
                                      double* grad_pred_jerk_out_dev);

/* The edit of :649-672 as a plan step (prepend_count_kernel, vertex_offsets_kernel, prepend_write_kernel): per path the first
 * requested waypoint goes where decision_dev has MRS_TG_IC_DROP_FIRST (and the path has one), and row 0 of initial_dev
 * [n_paths][4][4] comes in front where it has MRS_TG_IC_PREPEND, with stop_at 0.  waypoints_dev [n_vertices][4] and stop_at_dev
 * [n_vertices] (may be NULL: zeros) are addressed by vertex_offsets_dev [n_paths + 1], n_vertices = vertex_offsets[n_paths] as
 * the caller built it.  The result is packed as mrs_tg_plan_preprocess_path packs it: vertex_offsets_out_dev [n_paths + 1],
 * waypoints_out_dev (room for n_vertices + n_paths rows; the rows below vertex_offsets_out[n_paths] are written once, nothing
 * at or behind it), stop_at_out_dev and source_out_dev (may be NULL; the batch-wide input vertex, -1 for the prepended row).
 * Three launches (count, one workgroup sums, one lane per output vertex writes); no atomics, no waiting between workgroups.
 * A path may come out with no vertex or one: mrs_tg_plan_create refuses it, the caller fails it ("the path is empty").
 * MRS_TG_ERR_INVALID_ARG, before any launch: a missing mandatory pointer, a negative n_vertices, n_vertices + n_paths beyond
 * int32. */
int mrs_tg_plan_prepend_initial_condition(mrs_tg_plan* plan, const int32_t* vertex_offsets_dev, int32_t n_vertices,
                                          const double* waypoints_dev, const uint8_t* stop_at_dev, const int32_t* decision_dev,
                                          const double* initial_dev, int32_t* vertex_offsets_out_dev, double* waypoints_out_dev,
                                          uint8_t* stop_at_out_dev, int32_t* source_out_dev);
/* Its backward pass (prepend_vjp_kernel): grad_waypoints_edited_dev [n_vertices_edited][4] on the packed result, addressed by
 * vertex_offsets_edited_dev as the forward wrote it, gives grad_waypoints_out_dev [n_vertices][4] of the requested vertices (a
 * dropped vertex gets a zero row) and grad_initial_row_out_dev [n_paths][4], the gradient of row 0 of the state block (zero
 * where nothing was prepended).  Copies only; every element written exactly once. */
int mrs_tg_plan_prepend_initial_condition_vjp(mrs_tg_plan* plan, const int32_t* vertex_offsets_dev, int32_t n_vertices,
                                              const int32_t* decision_dev, const int32_t* vertex_offsets_edited_dev,
                                              int32_t n_vertices_edited, const double* grad_waypoints_edited_dev,
                                              double* grad_waypoints_out_dev, double* grad_initial_row_out_dev);

/* The pre-trajectory of a path stamped in the future (:801-840) as a plan step (splice_prediction_kernel), on samples where
 * they are; the batched form of mrs_tg_splice_prediction.  samples_dev [n_paths][sample_capacity][4], n_samples_dev and
 * status_dev (may be NULL: every path is live) are what a solve or a sampler left; decision_dev and sample_offset_dev (k) are
 * mrs_tg_plan_initial_condition's; prediction_age_dev [n_paths] = now - the stamp of the prediction held after the solve;
 * pred_position_dev [n_paths][pred_capacity][4] with n_pred_dev rows valid.  With k2 = int(floor((age - 0.01) / 0.2)) + 1: where
 * a path is live, MRS_TG_IC_FROM_FUTURE is set, k > 0 and k > k2, prediction rows 0 .. k-1 go in front of the n rows, in that
 * order, and n_samples_out = n + k.  If n + k > sample_capacity nothing of that path is written and the count n + k is still
 * reported.  k > n_pred (or a NaN age) sets MRS_TG_STATUS_INVALID_ARGS in status_out_dev [n_paths] (may be NULL, may be
 * status_dev; every other path passes its status on, 1 without status_dev) and leaves the path alone: the host function
 * refuses that case.  A path is left alone, rows and count, if its status is <= 0, if its n_samples is outside
 * [0, sample_capacity] (sample_capacity + 1: a sampler overflow), or if it needs no splice.
 * samples_out_dev may be samples_dev: the shift then walks the chunks of 64 rows from the last to the first, each chunk loading
 * all its rows before it stores any, and writes the prefix after the lowest chunk, which is correct for every k.  Out of place
 * the two arrays may not overlap; rows 0 .. n + k - 1 are written whole, and a live path that is left alone has its rows
 * copied.  In both forms no row at or behind the new count is written.  n_samples_out_dev may be n_samples_dev.  One wavefront
 * per path; no LDS, no atomics.  MRS_TG_ERR_INVALID_ARG, before any launch: a missing mandatory pointer, a negative
 * sample_capacity or pred_capacity, sample_capacity + pred_capacity beyond int32. */
int mrs_tg_plan_splice_prediction(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                  int32_t sample_capacity, const int32_t* status_dev, const int32_t* decision_dev,
                                  const int32_t* sample_offset_dev, const double* prediction_age_dev,
                                  const double* pred_position_dev, const int32_t* n_pred_dev, int32_t pred_capacity,
                                  double* samples_out_dev, int32_t* n_samples_out_dev, int32_t* status_out_dev);
/* Its backward pass (splice_prediction_vjp_kernel); n_samples_dev and status_dev are the forward's INPUTS.  Where the forward
 * spliced: grad_samples[i] = grad_out[i + k] for i < n and grad_pred_position[i] = grad_out[i] for i < k, zero everywhere else
 * that belongs to the path.  Where nothing was spliced grad_samples is the rows 0 .. n-1 of grad_out (none for a path with
 * status <= 0) and the prediction's rows are zero.  grad_out_dev, grad_samples_out_dev [n_paths][sample_capacity][4],
 * grad_pred_position_out_dev [n_paths][pred_capacity][4].  Copies only; every element written exactly once. */
int mrs_tg_plan_splice_prediction_vjp(mrs_tg_plan* plan, const int32_t* n_samples_dev, int32_t sample_capacity,
                                      const int32_t* status_dev, const int32_t* decision_dev, const int32_t* sample_offset_dev,
                                      const double* prediction_age_dev, const int32_t* n_pred_dev, int32_t pred_capacity,
                                      const double* grad_out_dev, double* grad_samples_out_dev,
                                      double* grad_pred_position_out_dev);

/* The vertices findTrajectory builds from a request (mrs_trajectory_generation.cpp:923-977), as a plan step
 * (MRS_TG_CAP_REQUEST; request_vertices_kernel, csrc/mrs_tg_request.hpp); the batched form of the
 * vertex construction of mrs_tg_optimize_paths' host loop, the same bits.  waypoints_dev [sum V][4] are the RAW waypoints of
 * the plan's paths; stop_at_dev [sum V] (may be NULL: none); has_state_dev [n_paths] (may be NULL: no path has a state) with
 * state_dev [n_paths][4][4], the block mrs_tg_plan_initial_condition writes: row 0 column 3 the heading, rows 1 .. 3 velocity,
 * acceleration and jerk of (x, y, z, heading); a block is read only where has_state is non-zero.  Per path of V vertices:
 *   last = has_state ? state[0][3] : raw[0][3];   for every vertex  h_i = unwrap(raw[i][3], last), last = h_i
 * (sradians::unwrap, fmod and additions: the host's bits), waypoints_out[i] = (x, y, z, h_i), mask[i][0] = 1,
 * values[i][0][:] = waypoints_out[i]; the first and the last vertex have mask[1 .. d] = 1; the first vertex of a path with a
 * state has mask[1 .. 3] = 1 (for d = 2 too) and values[1 .. 3][:] = state[1 .. 3][:]; a vertex between the ends with stop_at
 * has mask[1 .. 3] = 1; stop_at on an end changes nothing; every other mask byte is 0 and every other value +0.0.
 * waypoints_out_dev [sum V][4], fixed_mask_out_dev [sum V][5] and fixed_values_out_dev [sum V][5][4] may each be NULL, not all;
 * waypoints_out_dev may be waypoints_dev.  One launch, one wavefront per path, the chain a wave-uniform loop over chunks of 64
 * vertices; no LDS, no atomics, no workspace; every element written exactly once.
 * MRS_TG_ERR_INVALID_ARG, before any launch: waypoints_dev NULL, derivative_to_optimize outside 2 .. 4, has_state_dev without
 * state_dev, no output at all.  Device pointers (16-byte aligned), asynchronous on the context's stream. */
int mrs_tg_plan_request_vertices(mrs_tg_plan* plan, const double* waypoints_dev, const uint8_t* stop_at_dev,
                                 const uint8_t* has_state_dev, const double* state_dev, int32_t derivative_to_optimize,
                                 double* waypoints_out_dev, uint8_t* fixed_mask_out_dev, double* fixed_values_out_dev);
/* Its backward pass (request_vertices_vjp_kernel), every branch held fixed: the unwrap adds a piecewise-constant multiple of
 * 2 pi, so dh_i/draw_i = 1 and dh_i/d(state heading) = 0.  From grad_waypoints_dev [sum V][4] (on waypoints_out) and
 * grad_fixed_values_dev [sum V][5][4] (each may be NULL = zero, not both):
 *   grad_waypoints_out[i][:] = grad_waypoints[i][:] + grad_fixed_values[i][0][:]          (one addition)
 *   grad_state_out[p][1 .. 3][:] = grad_fixed_values[first vertex of p][1 .. 3][:] where the path has a state, else zeros;
 *   grad_state_out[p][0][:] = 0.
 * Upstreams on value slots the forward writes as constant zeros are dropped.  grad_waypoints_out_dev [sum V][4] and
 * grad_state_out_dev [n_paths][4][4] may each be NULL, not both.  One lane per vertex; every element written exactly once, zeros
 * included; no atomics. */
int mrs_tg_plan_request_vertices_vjp(mrs_tg_plan* plan, const uint8_t* has_state_dev, const double* grad_waypoints_dev,
                                     const double* grad_fixed_values_dev, double* grad_waypoints_out_dev,
                                     double* grad_state_out_dev);
/* The limits findTrajectory derives from a request (:981-1038; fallback != 0: findTrajectoryFallback's variant, :1252-1299), as a
 * plan step (request_limits_kernel, one lane per path); the plan contributes its path count and its context.
 *   constraints_dev [n_paths][12]  horizontal speed, acceleration, jerk; vertical ascending / descending speed; ascending /
 *                                  descending acceleration; ascending / descending jerk; heading speed, acceleration, jerk
 *   override_dev [n_paths][6]      override velocity h, v; acceleration h, v; jerk h, v, as the reference's override_max_*_
 *                                  members hold them (its callbacks put the horizontal jerk into the vertical member: that is
 *                                  the caller's business); may be NULL together with flags_dev
 *   flags_dev [n_paths]            MRS_TG_REQ_*; NULL = 0
 *   has_state_dev, state_dev       as mrs_tg_plan_request_vertices takes them
 * limits_out_dev [n_paths][9] = {v_h, v_v, v_hdg, a_h, a_v, a_hdg, j_h, j_v, j_hdg}.  A vertical limit is
 * (desc < asc) ? desc : asc (a tie takes the ascending value).  With MRS_TG_REQ_OVERRIDE and fallback == 0 the override replaces
 * the six horizontal and vertical values if can_change holds: true without a state, else hypot(vx, vy) < o[0],
 * hypot(ax, ay) < o[2], hypot(jx, jy) < o[4], |vz| < o[1], |az| < o[3], |jz| < o[5], all strict (a NaN refuses); with
 * fallback != 0 it replaces them unconditionally.  MRS_TG_REQ_RELAX_HEADING: the three heading limits are (double)FLT_MAX.
 * fallback != 0: afterwards entries 0 and 1 are multiplied by speed_factor, 3 and 4 by accel_factor.  hypot is the device's:
 * the decision can differ from the host's only for a state within an ulp of the override.  branch_out_dev [n_paths]
 * (MRS_TG_LIM_*; the *_DESCENDING bits say which side of a pair the constraints' minimum is, overridden or not).  Either output
 * may be NULL, not both.  MRS_TG_ERR_INVALID_ARG, before any launch: constraints_dev NULL, flags_dev without override_dev,
 * has_state_dev without state_dev, no output at all. */
int mrs_tg_plan_request_limits(mrs_tg_plan* plan, const double* constraints_dev, const double* override_dev,
                               const int32_t* flags_dev, const uint8_t* has_state_dev, const double* state_dev, int32_t fallback,
                               double speed_factor, double accel_factor, double* limits_out_dev, int32_t* branch_out_dev);
/* Its backward pass (request_limits_vjp_kernel), the branch word held fixed; fallback and the factors are the forward's.  With
 * g_k = grad_limits[k], times the fallback's factor on k = 0, 1, 3, 4: the entry that supplied limit k gets g_k -- the override
 * entry where MRS_TG_LIM_OVERRIDDEN is set, else the constraint (the winning side of a vertical pair); a relaxed heading limit
 * gives nothing; the state gets no gradient.  grad_constraints_out_dev [n_paths][12] and grad_override_out_dev [n_paths][6] may
 * each be NULL, not both; every element written exactly once, zeros included.  MRS_TG_ERR_INVALID_ARG: branch_dev or
 * grad_limits_dev NULL (no upstream), no output at all. */
int mrs_tg_plan_request_limits_vjp(mrs_tg_plan* plan, const int32_t* branch_dev, int32_t fallback, double speed_factor,
                                   double accel_factor, const double* grad_limits_dev, double* grad_constraints_out_dev,
                                   double* grad_override_out_dev);

/* Mutual clearance within groups of paths as a plan step (MRS_TG_CAP_MUTUAL_CLEARANCE; mutual_clearance_kernel,
 * csrc/mrs_tg_clearance.hpp): how close the UAVs of one swarm come to each other, when, and who the
 * neighbour is -- on the rows a sampler left, where they are.  The plan contributes its path count and its context; segments play
 * no part and every array is in the caller's path order.  The paths are partitioned into GROUPS, contiguous runs of paths:
 * group_offsets_dev [n_groups + 1] (int32; well-formed offsets start at 0, do not decrease and end at n_paths).  All paths share
 * the sampling dt: row r of path p sits at the common step first_step[p] + r (first_step_dev [n_paths] int32, NULL = all 0,
 * values in [-2^30, 2^30]).  samples_dev [n_paths][sample_capacity][4] and n_samples_dev [n_paths] are what a solve or a sampler
 * left; a path has n = min(n_samples, sample_capacity) live rows (a count of sample_capacity + 1 is sample_capacity rows), none
 * with status_dev (may be NULL) <= 0 -- such a path is neither a subject nor a neighbour.  For every live row (p, r) at step s and
 * every other path j of p's group with a live row at step s, with d = row_p - row_j and kappa = z_scale (finite, positive; 1.0
 * the Euclidean distance, below 1 vertical separation weighs less),
 *   c = sqrt((dx dx + dy dy) + (kappa dz)(kappa dz))        products and sums in this order, no fused multiply-add
 * and the row's clearance is the minimum over j, taken with a strict < from +inf in increasing j: a tie goes to the lowest path
 * index, a distance that is not a number never becomes a minimum.  Outputs, each may be NULL, not all:
 *   clearance_out_dev [n_paths][sample_capacity]      the minimum; +inf where no neighbour has a row at that step, in the rows
 *                                                     from n on and on dead paths (relu(R - c) needs no mask)
 *   partner_out_dev [n_paths][sample_capacity] int32  the neighbour's path index in the batch, -1 exactly where clearance is +inf
 *   min_clearance_out_dev [n_paths]                   the minimum over the path's rows, +inf without any
 *   argmin_out_dev [n_paths][2] int32                 the first row whose clearance is strictly below every row in front of it,
 *                                                     and its partner; {-1, -1} without any
 * One workgroup per path, one lane per row, the group's other paths the outer loop of a chunk of 64 rows; the per-path minimum
 * is combined in the order "smaller value, then lower row", which no split changes.  No atomics, no workspace; every output
 * element that belongs to the plan is written exactly once; the same bits on every call and for a path wherever its group sits
 * in the batch.  Group bounds are clamped into [0, n_paths] and every row index is checked against its path's live rows, so no
 * read leaves the plan's arrays whatever group_offsets_dev and first_step_dev hold; a path that offsets which are not
 * well-formed leave outside its group's range has no neighbours.  Out of scope: a path counts only on the steps where it has
 * rows ("hovers at its last row" is the caller's padding: repeat the row and raise n_samples); groups that are not contiguous.
 * MRS_TG_ERR_INVALID_ARG, before any launch: plan, n_samples_dev or group_offsets_dev NULL, samples_dev NULL with a positive
 * capacity, n_groups < 0, a negative sample_capacity, a z_scale that is not finite and positive, no output given, samples_dev
 * not 16-byte aligned or another array not aligned to its element.  n_paths == 0 or sample_capacity == 0: success, nothing is
 * launched or written.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_mutual_clearance(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev, int32_t sample_capacity,
                                 const int32_t* group_offsets_dev, int32_t n_groups, const int32_t* first_step_dev,
                                 const int32_t* status_dev, double z_scale, double* clearance_out_dev, int32_t* partner_out_dev,
                                 double* min_clearance_out_dev, int32_t* argmin_out_dev);
/* Backward pass of mrs_tg_plan_mutual_clearance (mutual_clearance_vjp_kernel), the partners held fixed:
 * given grad_clearance_dev [n_paths][sample_capacity] = dL/dclearance and partner_dev, the forward's partner_out_dev (an input),
 * writes grad_samples_out_dev [n_paths][sample_capacity][4] = dL/dsamples: column 3 zero, rows from n on zero, dead paths zero.
 * For a row (i, .) at step s with upstream g, partner j and d = row_i - row_j,
 *   g dc/drow_i = (g (dx / c), g (dy / c), g ((kappa (kappa dz)) / c))    each quotient rounded, then the product
 *   g dc/drow_j = 0.0 - that, entry by entry.
 * Row (j, r) at step s has one accumulator per coordinate: it starts at 0.0 and takes first the row's own term against its own
 * partner, then, in increasing path index i over the group with i != j, the second form of every i whose row at step s names j
 * as its partner; every addition is one rounded addition.  Exactly 0 come from: g == 0 (so the +inf rows never make a NaN),
 * c == 0 (coincident rows), a partner entry that is -1, outside the row's own group, the row's own path, or a path without a
 * live row at that step -- none of which is dereferenced.  No gradient flows through the choice of the partner.  A gather, one
 * lane per output row: deterministic, no atomics, no workspace, every element written exactly once, the same bits on every call
 * and wherever the group sits in the batch.  grad_samples_out_dev may not overlap an input.  The argument checks are the
 * forward's, with partner_dev, grad_clearance_dev and grad_samples_out_dev (16-byte aligned) required. */
int mrs_tg_plan_mutual_clearance_vjp(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                     int32_t sample_capacity, const int32_t* group_offsets_dev, int32_t n_groups,
                                     const int32_t* first_step_dev, const int32_t* status_dev, double z_scale,
                                     const int32_t* partner_dev, const double* grad_clearance_dev, double* grad_samples_out_dev);

/* Clearance from static obstacles as a plan step (MRS_TG_CAP_OBSTACLE_CLEARANCE; obstacle_clearance_kernel,
 * csrc/mrs_tg_obstacle.hpp): how close every row a sampler left comes to a map, and which obstacle of
 * the map that is.  The plan contributes its path count and its context; segments play no part and every array is in the
 * caller's path order.  An obstacle is four doubles (x, y, z, radius): a sphere, or with radius 0 a point of a cloud.  The
 * obstacles live in one array obstacles_dev [n_obstacles][4], partitioned into SETS, contiguous runs: set_offsets_dev
 * [n_sets + 1] (int32; well-formed offsets start at 0, do not decrease and end at n_obstacles).  path_set_dev [n_paths] (int32)
 * names the set each path sees; NULL = every path sees set 0.  A path sees no obstacle when its path_set entry is outside
 * [0, n_sets), when its set is empty or when it is dead.  samples_dev [n_paths][sample_capacity][4] and n_samples_dev [n_paths]
 * are what a solve or a sampler left; a path has n = min(n_samples, sample_capacity) live rows (a count of sample_capacity + 1
 * is sample_capacity rows), none with status_dev (may be NULL) <= 0.  For every live row (x, y, z, .) of path p and every
 * obstacle k of p's set, with kappa = z_scale (finite, positive; 1.0 the Euclidean distance, below 1 vertical separation
 * weighs less),
 *   dx = x - ox,  dy = y - oy,  dz = kappa (z - oz)
 *   s = sqrt((dx dx + dy dy) + dz dz),  c = s - radius      products and sums in this order, no fused multiply-add
 * c is signed: negative inside a sphere.  The row's clearance is the minimum of c over k, taken with a strict < from +inf in
 * increasing k: a tie goes to the lowest obstacle index, a c that is not a number never becomes a minimum.  Coordinates and
 * radii are ordinary data: a NaN coordinate makes that obstacle lose, an infinite radius is what the arithmetic makes of it.
 * Outputs, each may be NULL, not all:
 *   clearance_out_dev [n_paths][sample_capacity]      the minimum; +inf where the path sees no obstacle, in the rows from n on
 *                                                     and on dead paths (relu(R - c) needs no mask)
 *   nearest_out_dev [n_paths][sample_capacity] int32  the nearest obstacle's index in the WHOLE obstacles array, -1 exactly where
 *                                                     clearance is +inf
 *   min_clearance_out_dev [n_paths]                   the minimum over the path's rows, +inf without any
 *   argmin_out_dev [n_paths][2] int32                 the first row whose clearance is strictly below every row in front of it,
 *                                                     and its obstacle; {-1, -1} without any
 * One workgroup per path, one lane per row, the obstacles of the path's set the inner loop in increasing index, read as
 * wavefront-uniform data; the per-path minimum is combined in the order "smaller value, then lower row", which no split
 * changes.  No atomics, no workspace; every output element that belongs to the plan is written exactly once; the same bits on
 * every call and for a path wherever it sits in the batch and wherever its set sits in the array.  Set bounds are clamped into
 * [0, n_obstacles] with end >= begin, so no read leaves the obstacle array whatever set_offsets_dev and path_set_dev hold.  Out
 * of scope: a gradient with respect to the obstacles (a static map); a spatial index over them is
 * mrs_tg_plan_field_clearance's voxel grid, built once from this step; a small batch against a large
 * map uses one workgroup per path and so a part of the device.
 * MRS_TG_ERR_INVALID_ARG, before any launch: plan, n_samples_dev or set_offsets_dev NULL, samples_dev NULL with a positive
 * capacity, obstacles_dev NULL with n_obstacles > 0, a negative n_obstacles, n_sets or sample_capacity, a z_scale that is not
 * finite and positive, no output given, samples_dev or obstacles_dev not 16-byte aligned or another array not aligned to its
 * element.  n_paths == 0 or sample_capacity == 0: success, nothing is launched or written.  n_obstacles == 0 or n_sets == 0: the
 * kernel runs and writes +inf / -1 everywhere.  Device pointers, asynchronous on the context's stream. */
int mrs_tg_plan_obstacle_clearance(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                   int32_t sample_capacity, const double* obstacles_dev, int32_t n_obstacles,
                                   const int32_t* set_offsets_dev, int32_t n_sets, const int32_t* path_set_dev,
                                   const int32_t* status_dev, double z_scale, double* clearance_out_dev,
                                   int32_t* nearest_out_dev, double* min_clearance_out_dev, int32_t* argmin_out_dev);
/* Backward pass of mrs_tg_plan_obstacle_clearance (obstacle_clearance_vjp_kernel), the nearest obstacles
 * held fixed: given grad_clearance_dev [n_paths][sample_capacity] = dL/dclearance and nearest_dev, the forward's nearest_out_dev
 * (an input), writes grad_samples_out_dev [n_paths][sample_capacity][4] = dL/dsamples: column 3 zero, rows from n on zero, dead
 * paths zero.  For a live row with upstream g, nearest obstacle k and dx, dy, dz, s as in the forward,
 *   dL/drow = (g (dx / s), g (dy / s), g ((kappa dz) / s))      each quotient rounded, then the product.
 * Exactly 0 come from: g == 0 (so the +inf rows never make a NaN), s == 0 (a row on a centre), a nearest entry that is -1 or
 * outside the path's own clamped set -- none of which dereferences an obstacle.  No gradient flows through the choice of the
 * obstacle, and there is none with respect to the obstacles.  One lane per output row: deterministic, no atomics, no workspace,
 * every element written exactly once, the same bits on every call and wherever the path sits in the batch.
 * grad_samples_out_dev may not overlap an input.  The argument checks are the forward's, with nearest_dev, grad_clearance_dev
 * and grad_samples_out_dev (16-byte aligned) required. */
int mrs_tg_plan_obstacle_clearance_vjp(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                       int32_t sample_capacity, const double* obstacles_dev, int32_t n_obstacles,
                                       const int32_t* set_offsets_dev, int32_t n_sets, const int32_t* path_set_dev,
                                       const int32_t* status_dev, double z_scale, const int32_t* nearest_dev,
                                       const double* grad_clearance_dev, double* grad_samples_out_dev);

/* Clearance from a voxel distance field as a plan step (MRS_TG_CAP_FIELD_CLEARANCE; field_clearance_kernel,
 * csrc/mrs_tg_field.hpp): how close every row a sampler left comes to a static map given as a grid of
 * signed distances (an ESDF), looked up by trilinear interpolation -- eight voxel reads per row whatever the size of the map,
 * where mrs_tg_plan_obstacle_clearance walks its list of obstacles per row.  The plan contributes its path count and its
 * context; segments play no part and every array is in the caller's path order.  fields_dev is [n_fields][nz][ny][nx] doubles,
 * x fastest: n_fields grids of ONE geometry (host struct) stacked in one array.  The value with indices (i, j, k) sits at
 * origin + (i hx, j hy, k hz): the grid is node-centred, and a caller with cell-centred voxels passes the centre of voxel 0 as
 * the origin; a 2-D map is passed as two equal layers.  path_field_dev [n_paths] (int32) names the grid each path sees; NULL =
 * every path sees grid 0; an entry outside [0, n_fields) = the path sees none.  samples_dev [n_paths][sample_capacity][4] and
 * n_samples_dev [n_paths] are what a solve or a sampler left; a path has n = min(n_samples, sample_capacity) live rows (a count
 * of sample_capacity + 1 is sample_capacity rows), none with status_dev (may be NULL) <= 0.  For a live row (x, y, z, .) of a path
 * that sees grid f, in this order and with no fused multiply-add:
 *   ux = (x - ox) / hx, uy, uz alike                         a true division
 *   inside  <=>  0 <= u && u <= n - 1 on every axis          tested in double: a NaN fails, a huge u is never made an integer
 *   i = (int)ux, lowered to nx - 2 when above it;  tx = ux - (double)i     (the upper face belongs to the last cell, tx = 1)
 *   lerp(a, b, t) = a + t (b - a);  fIJK the voxel at (i + I, j + J, k + K)
 *   c00 = lerp(f000, f100, tx), c10 = lerp(f010, f110, tx), c01 = lerp(f001, f101, tx), c11 = lerp(f011, f111, tx)
 *   c0 = lerp(c00, c10, ty), c1 = lerp(c01, c11, ty), clearance = lerp(c0, c1, tz)
 *   gx = lerp(lerp(f100 - f000, f110 - f010, ty), lerp(f101 - f001, f111 - f011, ty), tz) / hx
 *   gy = lerp(lerp(f010 - f000, f110 - f100, tx), lerp(f011 - f001, f111 - f101, tx), tz) / hy
 *   gz = lerp(lerp(f001 - f000, f101 - f100, tx), lerp(f011 - f010, f111 - f110, tx), ty) / hz
 *   cell = ((f nz + k) ny + j) nx + i                        the low corner's index in the WHOLE fields array
 * Voxel values are ordinary data: an infinite or NaN voxel gives what the arithmetic makes of it; a NaN clearance is written
 * as it is and never becomes a minimum.  Outputs, each may be NULL, not all:
 *   clearance_out_dev [n_paths][sample_capacity]       the interpolant; outside_value (any double: +inf for "unknown is free",
 *                                                      a negative value for "unknown is occupied") for a live row that is not
 *                                                      inside; +inf in the rows from n on, on dead paths and on paths that see
 *                                                      no grid (relu(R - c) needs no mask)
 *   cell_out_dev [n_paths][sample_capacity] int32      the cell; -1 wherever the row is not a live row inside its path's grid
 *   gradient_out_dev [n_paths][sample_capacity][4]     (gx, gy, gz, 0): the field's gradient at the row; zeros wherever cell = -1
 *   min_clearance_out_dev [n_paths]                    the minimum over the path's rows, +inf without any
 *   argmin_out_dev [n_paths][2] int32                  {row, cell} of the first row whose clearance is strictly below every row in
 *                                                      front of it, starting from +inf; {-1, -1} without any.  An outside_value
 *                                                      row takes part like any other and reports cell = -1
 * One workgroup per path, one lane per row; the per-path minimum is combined in the order "smaller value, then lower row",
 * which no split changes.  No atomics, no workspace; every output element that belongs to the plan is written exactly once;
 * the same bits on every call and for a path wherever it sits in the batch.  Out of scope: float32 fields; a gradient with
 * respect to the field; interpolation smoother than trilinear; splitting one path over several workgroups.  (The field itself:
 * from an occupancy grid mrs_tg_field_from_occupancy builds it on the device; from a list of obstacles it IS
 * mrs_tg_plan_obstacle_clearance's output over the nodes)
 * MRS_TG_ERR_INVALID_ARG, before any launch: plan, n_samples_dev or geometry NULL, fields_dev NULL with n_fields > 0,
 * samples_dev NULL with a positive capacity, a negative sample_capacity or n_fields, a dim below 2, a spacing that is not
 * finite and positive, an origin that is not finite, n_fields nz ny nx above 2^31 - 1 (a cell is an int32), no output given,
 * samples_dev or gradient_out_dev not 16-byte aligned or another array not aligned to its element.  n_paths == 0 or
 * sample_capacity == 0: success, nothing is launched or written.  n_fields == 0: the kernel runs and writes +inf / -1 (and
 * zeros) everywhere.  Device pointers except geometry, asynchronous on the context's stream. */
typedef struct mrs_tg_field_geometry {
  double origin[3];  /* x, y, z of node (0, 0, 0) */
  double spacing[3]; /* hx, hy, hz: finite, positive */
  int32_t dims[3];   /* nx, ny, nz: each >= 2 */
  int32_t n_fields;  /* >= 0: grids of this geometry stacked in one array */
} mrs_tg_field_geometry;
int mrs_tg_plan_field_clearance(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                int32_t sample_capacity, const double* fields_dev, const mrs_tg_field_geometry* geometry,
                                const int32_t* path_field_dev, const int32_t* status_dev, double outside_value,
                                double* clearance_out_dev, int32_t* cell_out_dev, double* gradient_out_dev,
                                double* min_clearance_out_dev, int32_t* argmin_out_dev);
/* Backward pass of mrs_tg_plan_field_clearance (field_clearance_vjp_kernel), the cells held fixed: given
 * grad_clearance_dev [n_paths][sample_capacity] = dL/dclearance and cell_dev, the forward's cell_out_dev (an input), writes
 * grad_samples_out_dev [n_paths][sample_capacity][4] = dL/dsamples = (g gx, g gy, g gz, 0): rows from n on zero, dead paths
 * zero.  gx, gy, gz are recomputed from the row and the recorded cell as in the forward, with t = u - (double)i NOT clamped
 * again: for the same inputs g * gradient_out_dev and this output are the same bits.  Exactly 0 come from: g == 0 (so the +inf
 * rows never make a NaN), cell = -1, a cell that decodes to a grid other than the path's own, a cell that decodes to i, j, k
 * outside [0, n - 2] -- none of which dereferences a voxel.  There is no gradient with respect to the field, and none through
 * the choice of the cell.  One lane per output row: deterministic, no atomics, no workspace, every element written exactly
 * once, the same bits on every call and wherever the path sits in the batch.  The argument checks are the forward's, with
 * cell_dev, grad_clearance_dev and grad_samples_out_dev (16-byte aligned) required; grad_samples_out_dev may not overlap an
 * input (MRS_TG_ERR_INVALID_ARG). */
int mrs_tg_plan_field_clearance_vjp(mrs_tg_plan* plan, const double* samples_dev, const int32_t* n_samples_dev,
                                    int32_t sample_capacity, const double* fields_dev, const mrs_tg_field_geometry* geometry,
                                    const int32_t* path_field_dev, const int32_t* status_dev, const int32_t* cell_dev,
                                    const double* grad_clearance_dev, double* grad_samples_out_dev);

/* The distance field from an occupancy grid (MRS_TG_CAP_FIELD_FROM_OCCUPANCY; edt_x_kernel, edt_y_kernel, edt_z_kernel,
 * csrc/mrs_tg_edt.hpp): an exact Euclidean distance transform on the device, from what a mapping stack
 * publishes to what mrs_tg_plan_field_clearance reads, in the same layout and geometry.  Keyed on the context, not on a plan: a
 * map has no paths.  occupancy_dev is [n_fields][nz][ny][nx] uint8, x fastest, node-centred, grids of ONE geometry stacked; a
 * voxel is OCCUPIED when its byte is non-zero (what "unknown" means is the caller's business).  fields_out_dev is
 * [n_fields][nz][ny][nx] doubles.  With the weights
 *   wx = hx hx,  wy = hy hy,  wz = (z_scale hz) (z_scale hz)                      computed once on the host
 * the squared distance between two nodes of one grid with integer offsets di, dj, dk is
 *   q = (wx (double)(di di) + wy (double)(dj dj)) + wz (double)(dk dk)           in this order, nothing fused
 * D_occ(v) is the minimum of q over the occupied nodes of v's own grid, +inf where there is none; D_free(v) the same over the
 * free nodes; grids never see each other.  With rt(D) = min(sqrt(D), max_distance), sqrt correctly rounded:
 *   flags = 0                  a free node gets rt(D_occ), an occupied node 0.0
 *   MRS_TG_FIELD_SIGNED        a free node gets rt(D_occ), an occupied node -rt(D_free)
 * The result is this definition in every bit, whatever the algorithm (three separable passes with an outward scan per node:
 * csrc/mrs_tg_edt.hpp holds the argument).  z_scale is the weight on the vertical separation of the clearance steps.
 * max_distance is positive and may be +inf.  THE TRAP: with +inf an all-free or all-occupied grid yields +-inf voxels, and
 * lerp(inf, inf, t) is NaN in mrs_tg_plan_field_clearance; a caller who looks such a field up passes a finite cap (which also
 * bounds the scan, and so the cost, on a sparse map).  The origin plays no part in the values and is checked like the rest.
 * A dim may not exceed MRS_TG_FIELD_MAX_DIM (a line of the y and z passes is staged in LDS).  The passes run in place in
 * fields_out_dev: no workspace, signed or not.  No atomics; occupancy_dev is only read; every output element is written; the same input gives the same bits on every call.
 * Out of scope: the index of the nearest occupied voxel; float32 fields; sub-voxel surfaces; a gradient of anything (occupancy
 * is discrete).  (A map that changes inside a box: mrs_tg_field_update_region, below.)
 * MRS_TG_ERR_INVALID_ARG, with the context's last error set and nothing launched: ctx or geometry NULL; occupancy_dev or
 * fields_out_dev NULL with voxels to process; a negative n_fields, a dim below 2 or above MRS_TG_FIELD_MAX_DIM, a spacing that
 * is not finite and positive, an origin that is not finite, n_fields nz ny nx above 2^31 - 1; a z_scale that is not finite and
 * positive; a max_distance that is NaN or <= 0; unknown flag bits; fields_out_dev not 8-byte aligned or overlapping
 * occupancy_dev.  n_fields == 0: success, nothing is launched or written.  Device pointers except geometry, asynchronous on
 * the context's stream. */
#define MRS_TG_FIELD_SIGNED 1
#define MRS_TG_FIELD_MAX_DIM 1024
int mrs_tg_field_from_occupancy(mrs_tg_ctx* ctx, const uint8_t* occupancy_dev, const mrs_tg_field_geometry* geometry,
                                double z_scale, double max_distance, int32_t flags, double* fields_out_dev);

/* The distance field brought up to date after the occupancy changed inside a box (MRS_TG_CAP_FIELD_UPDATE_REGION;
 * edt_region_x_kernel, edt_region_y_kernel, edt_region_z_kernel, csrc/mrs_tg_edt_region.hpp): what a
 * mapping stack that rewrites a small box of voxels per scan calls instead of a full rebuild.  occupancy_dev is the NEW
 * occupancy of the whole stack, in mrs_tg_field_from_occupancy's layout; fields_inout_dev holds the field of the OLD occupancy,
 * built with the SAME z_scale, max_distance and flags; region names one grid of the stack and the box lo .. hi (x, y, z node
 * indices, inclusive) that holds every voxel of that grid whose byte may differ between the two (a voxel outside it that
 * differs makes the result undefined near it; the other grids must be unchanged or are the caller's to update).  After the call
 * fields_inout_dev holds, in every bit, what mrs_tg_field_from_occupancy gives for the new occupancy.
 * With T = nextafter(max_distance max_distance, +inf) the REACH of axis a is the largest d >= 0 with w_a (double)(d d) < T, held
 * to dims[a] - 1 (and equal to it with max_distance = +inf).  The CORE is the box grown by the reach on either side of every
 * axis, clipped to the grid: the only nodes whose value can differ, and the only elements of fields_inout_dev that are written,
 * each exactly once.  The WINDOW is the core grown by the reach once more, clipped: the only occupancy that is read.  The three
 * passes of the full transform run on the window through workspace_dev, which holds [window nz][window ny][core nx] doubles
 * (workspace_bytes of mrs_tg_field_update_query, 8-byte aligned, the caller's: the call stays asynchronous and allocates
 * nothing).  When the window is the whole grid on every axis (whole_grid; always so with max_distance = +inf) the full
 * transform runs on that one grid instead, in place: no workspace is needed (workspace_bytes = 0, workspace_dev may be NULL),
 * and the core is reported as -- and is -- the whole grid.  Both routes are timed as kernel id 41, from first launch to last.
 * No atomics; occupancy_dev is only read; the same input gives the same bits on every call.
 * mrs_tg_field_update_query is host only: it needs no context, touches no device and fills *out from the geometry, z_scale,
 * max_distance and region alone (the error text goes to the global last error, mrs_tg_last_error(NULL)).
 * MRS_TG_ERR_INVALID_ARG, with the last error set and nothing launched: everything mrs_tg_field_from_occupancy refuses (with
 * fields_inout_dev in the place of fields_out_dev); n_fields == 0 (there is no grid to update); region or out NULL; field
 * outside [0, n_fields); lo > hi or an index outside the grid on any axis; when a workspace is needed, workspace_dev NULL, not
 * 8-byte aligned, workspace_bytes below the query's, or the workspace overlapping occupancy_dev or fields_inout_dev.  Device
 * pointers except geometry and region, asynchronous on the context's stream. */
typedef struct mrs_tg_field_region {
  int32_t field;        /* grid of the stack */
  int32_t lo[3], hi[3]; /* x, y, z node indices, inclusive */
} mrs_tg_field_region;
typedef struct mrs_tg_field_update_info {
  int32_t reach[3], core_lo[3], core_hi[3], window_lo[3], window_hi[3], whole_grid;
  int64_t workspace_bytes;
} mrs_tg_field_update_info;
int mrs_tg_field_update_query(const mrs_tg_field_geometry* geometry, double z_scale, double max_distance,
                              const mrs_tg_field_region* region, mrs_tg_field_update_info* out);
int mrs_tg_field_update_region(mrs_tg_ctx* ctx, const uint8_t* occupancy_dev, const mrs_tg_field_geometry* geometry,
                               double z_scale, double max_distance, int32_t flags, const mrs_tg_field_region* region,
                               void* workspace_dev, int64_t workspace_bytes, double* fields_inout_dev);

/* Duration in milliseconds of the most recent launch of a kernel, from the start and end time stamps of that very dispatch
 * (the events are attached to the kernel launch itself, hipExtLaunchKernelGGL: what rocprofv3 --kernel-trace reports for
 * it) -- requires mrs_tg_set_profiling(ctx, 1).  kernel_id: 0 block assembly, 1 linear solve, 2 nonlinear outer loop,
 * 3 backward pass of the solve (mrs_tg_plan_solve_vjp), 4 backward pass of the maxima (mrs_tg_plan_segment_maxima_vjp),
 * 5 backward pass of the sampler (mrs_tg_plan_sample_states_vjp), 6 evaluation at given times (mrs_tg_plan_evaluate),
 * 7 its backward pass (mrs_tg_plan_evaluate_vjp), 8 deviation from the waypoint path (mrs_tg_plan_path_deviation),
 * 9 its backward pass (mrs_tg_plan_path_deviation_vjp), 10 the segment-time estimate as a plan step
 * (mrs_tg_plan_estimate_times; inside a solve the estimate is not timed), 11 its backward pass
 * (mrs_tg_plan_estimate_times_vjp), 12 waypoint passage (mrs_tg_plan_waypoint_passage), 13 its backward pass
 * (mrs_tg_plan_waypoint_passage_vjp), 14 the Baca estimate as a plan step (mrs_tg_plan_estimate_times_baca), 15 its backward
 * pass (mrs_tg_plan_estimate_times_baca_vjp), 16 the length gate (mrs_tg_plan_length_gate), 17 the heading unwrap
 * (mrs_tg_plan_unwrap_headings), 18 the fallback sampler (mrs_tg_plan_fallback_sample), 19 its backward pass
 * (mrs_tg_plan_fallback_sample_vjp), 20 path thinning (mrs_tg_plan_preprocess_path), 21 mid-point subdivision
 * (mrs_tg_plan_insert_midpoints; both timed from their first launch to their last), 22 their backward pass
 * (mrs_tg_plan_path_edit_vjp), 23 the heading along the direction of travel (mrs_tg_plan_travel_heading), 24 its backward pass
 * (mrs_tg_plan_travel_heading_vjp), 25 the initial condition (mrs_tg_plan_initial_condition), 26 the prepended waypoint
 * (mrs_tg_plan_prepend_initial_condition, timed from its first launch to its last), 27 the prediction splice
 * (mrs_tg_plan_splice_prediction), 28, 29, 30 their backward passes (mrs_tg_plan_splice_prediction_vjp,
 * mrs_tg_plan_initial_condition_vjp, mrs_tg_plan_prepend_initial_condition_vjp), 31 the request's vertices
 * (mrs_tg_plan_request_vertices), 32 their backward pass (mrs_tg_plan_request_vertices_vjp), 33 the request's limits
 * (mrs_tg_plan_request_limits), 34 their backward pass (mrs_tg_plan_request_limits_vjp), 35 the mutual clearance
 * (mrs_tg_plan_mutual_clearance), 36 its backward pass (mrs_tg_plan_mutual_clearance_vjp), 37 the clearance from obstacles
 * (mrs_tg_plan_obstacle_clearance), 38 its backward pass (mrs_tg_plan_obstacle_clearance_vjp), 39 the clearance from a
 * distance field (mrs_tg_plan_field_clearance), 40 its backward pass (mrs_tg_plan_field_clearance_vjp), 41 the
 * distance field from an occupancy grid (mrs_tg_field_from_occupancy, timed from its first launch to its last): forty-two ids,
 * 0 .. 41.
 * Blocks until that launch has finished. */
int mrs_tg_set_profiling(mrs_tg_ctx* ctx, int enabled); /* switching it on starts a new series */
int mrs_tg_last_kernel_ms(mrs_tg_ctx* ctx, int kernel_id, float* ms_out);
/* The durations of the newest timed launches of the series (at most 512 are kept, oldest first; launches may be queued
 * back to back, every one carries its own pair of events).  Returns the number written (<= capacity) or a negative
 * MRS_TG_ERR_*.  Blocks until those launches have finished. */
int mrs_tg_kernel_ms_history(mrs_tg_ctx* ctx, int kernel_id, float* ms_out, int capacity);

/* Diagnostics (ABI 4): the names of the kernels the CALLING THREAD has launched through this library since its last
 * mrs_tg_kernel_trace_reset(), oldest first; at most the newest 32 are kept.  names_out receives pointers to static
 * strings ("solve_quad_group_kernel", ...).  Returns the number written.  A test or a benchmark can state which kernels a
 * call ran instead of inferring them from the batch size. */
void mrs_tg_kernel_trace_reset(void);
int mrs_tg_kernel_trace(const char** names_out, int capacity);
/* (ABI 5) The routing table, asked of the routers: the names of the kernels a call WOULD launch for this plan under these
 * options, in launch order -- the calling thread runs the same launch functions in a dry mode in which every size rule,
 * environment knob and hint takes effect and nothing is enqueued (no device work, no argument is dereferenced).
 * group_size 0: what mrs_tg_plan_solve(plan, ..., opt, ...) launches; 1 .. 16: what one dispatch of
 * mrs_tg_bound_solve_launch_group carrying that many batches of this plan launches.  names_out receives pointers to static
 * strings; returns the number written (<= capacity) or a negative MRS_TG_ERR_*.  Resets the calling thread's kernel trace.
 * tests/test_gpu_routing.py pins the route of every BASELINE config and of the nodelet's defaults with it; DESIGN.md section 4's
 * table is its output (scripts/routing_table.py). */
int mrs_tg_plan_explain(mrs_tg_plan* plan, const mrs_tg_options* opt, int32_t group_size, const char** names_out, int32_t capacity);

/* ---- single-path convenience mirroring findTrajectory()'s signature ------------------------- */

typedef struct mrs_tg_waypoint {
  double coords[4]; /* x, y, z, heading  (Waypoint_t, src/mrs_trajectory_generation.cpp:66-70) */
  uint8_t stop_at;
} mrs_tg_waypoint;

typedef struct mrs_tg_initial_state { /* the TrackerCommand fields read at src/...cpp:925-957 */
  double heading;
  double velocity[4], acceleration[4], jerk[4]; /* xyz + heading rate / acceleration / jerk */
} mrs_tg_initial_state;

/* findTrajectory(waypoints, initial_state, sampling_dt, relax_heading) for one path
 * (src/mrs_trajectory_generation.cpp:857-1209), the WHOLE function: builds the vertices (:923-977), estimates the segment
 * times and the Baca total (:1046-1056), optimises, samples, and applies BOTH of the reference's gates -- the accept / reject
 * rule on the nlopt code (:1138-1149) and the temporal sanity check of the sampled trajectory against the Baca estimate
 * (:1178-1199, opt->max_trajectory_len_factor / min_trajectory_len_factor).  limits9 as above.  Returns MRS_TG_OK and
 * *n_samples_out > 0 exactly where the reference returns the states; *n_samples_out = 0 where it returns {} (status_out,
 * seg_times_out and coeffs_out still hold what was computed; mrs_tg_last_error(ctx) has the reference's message and
 * mrs_tg_find_trajectory_info says which gate).  samples_out [sample_capacity][4]; a trajectory with more samples than that
 * which passes the gates is reported as sample_capacity + 1: that count is a lower bound of the real one, so the upper side of
 * the sanity check still applies to it (already too long is too long) and the lower side does not (an overflow is never "too
 * short").  A runaway of the feasibility scaling (MRS_TG_RUNAWAY_TIME_FACTOR) is answered as in the reference, by the upper
 * side of the sanity check, where that side runs: sampling_dt > 0, samples_out given and max_trajectory_len_factor > 0 (the
 * solve then runs under MRS_TG_FLAG_REFERENCE_STATUS).  Where it does not run -- no sampling, or the factor <= 0, a switch the
 * reference does not have -- the product's own rule answers: status MRS_TG_STATUS_ROUNDOFF_LIMITED, MRS_TG_FIND_REJECTED_CODE,
 * no samples.  initial_state may be NULL. */
int mrs_tg_find_trajectory(mrs_tg_ctx* ctx, const mrs_tg_waypoint* waypoints, int32_t n_waypoints,
                           const mrs_tg_initial_state* initial_state, const double* limits9,
                           const mrs_tg_options* opt, int32_t relax_heading, double* seg_times_out,
                           double* coeffs_out, int32_t* status_out, int32_t* n_samples_out, double* samples_out);

/* (ABI 5) What the context's most recent mrs_tg_find_trajectory decided: *rejection_out = one of MRS_TG_FIND_*, and
 * *baca_total_time_out = initial_total_time_baca (:1048-1056) of that path -- the figure the reference prints beside its
 * "estimated/final trajectory length ratio" (:1201-1203).  Either pointer may be NULL. */
enum {
  MRS_TG_FIND_ACCEPTED = 0,
  MRS_TG_FIND_REJECTED_CODE = 1,      /* the optimiser's code is one the nodelet rejects (:1146-1149) */
  MRS_TG_FIND_REJECTED_TOO_LONG = 2,  /* "the final trajectory sampling is too long" (:1178-1186) */
  MRS_TG_FIND_REJECTED_TOO_SHORT = 3  /* "the final trajectory sampling is too short" (:1188-1196) */
};
int mrs_tg_find_trajectory_info(const mrs_tg_ctx* ctx, int32_t* rejection_out, double* baca_total_time_out);

/* (ABI 5) estimateSegmentTimesBaca (src/eth_trajectory_generation/vertex.cpp:301-485) for one path, as findTrajectory calls it
 * (:1048-1049; also the clock of the fallback sampler, :1309): waypoints [n_waypoints][4] with headings already unwrapped
 * along the path (:935), limits9 as above (after relax_heading), seg_times_out [n_waypoints - 1].  Host arithmetic, no device. */
int mrs_tg_estimate_times_baca(const double* waypoints, int32_t n_waypoints, const double* limits9, double* seg_times_out);

/* ---- path-policy layer: optimize() around findTrajectory(), for a batch of paths ------------- */

/* Parameters of the reference's policy layer (config/public/trajectory_generation.yaml; defaults by
 * mrs_tg_default_policy_options). */
typedef struct mrs_tg_policy_options {
  mrs_tg_options solver;               /* derivative, time allocation, sampling_dt ... of findTrajectory */
  int32_t check_deviation_enabled;     /* check_trajectory_deviation/enabled */
  double max_deviation;                /* check_trajectory_deviation/max_deviation [m] */
  int32_t max_deviation_iterations;    /* check_trajectory_deviation/max_iterations */
  int32_t max_deviation_first_segment; /* max_deviation_first_segment_ (src/...cpp:874-878) */
  double min_waypoint_distance;        /* preprocessPath (:484) */
  int32_t path_straightener_enabled;   /* path_straightener/... (:448-477) */
  double path_straightener_max_deviation, path_straightener_max_hdg_deviation;
  double max_trajectory_len_factor, min_trajectory_len_factor; /* length sanity check (:1178-1199) */
  int32_t fallback_sampling;           /* use findTrajectoryFallback (:1215-1395) instead of the optimiser */
  double fallback_speed_factor, fallback_accel_factor, fallback_stopping_time;
  int32_t override_heading_atan2;      /* getTrajectoryReference (:1582-1597) */
  int32_t reserved_;
  double max_execution_time_s;         /* max_execution_time (:2008-2033); <= 0: none.  As optimize() does (:702-716, :754-768):
                                          a round that starts while overtime() holds runs the fallback sampler for the paths
                                          still active (they succeed, "executing fallback sampling, we are running over time");
                                          otherwise the solver's max_time_s becomes 2 * 0.95 * time left (:899), and paths whose
                                          solve comes back after the deadline fail, as findTrajectory's own checks make the
                                          nodelet give up (:1085, 1156, 1171, 1516-1522).  fallback_sampling = 1 never looks
                                          at the clock */
} mrs_tg_policy_options;

void mrs_tg_default_policy_options(mrs_tg_policy_options* opt);

/* MrsTrajectoryGeneration::optimize() (src/mrs_trajectory_generation.cpp:620-851) for n_paths independent
 * paths: preprocessPath, solve (all still-active paths of a round in ONE batched GPU call), Baca length
 * sanity check, validateTrajectorySpatial, mid-point insertion into unsafe segments, re-solve -- up to
 * max_deviation_iterations rounds.  Tf is absent; the initial condition of stamped paths and the prediction splice are
 * mrs_tg_prepare_initial_condition / mrs_tg_splice_prediction below, around this call.
 *   wp_offsets [n_paths+1] CSR over `waypoints`; the first waypoint of a path is its initial condition when
 *   has_initial_state[p] != 0 (then initial_states[p] supplies the derivatives, :946-957).
 *   limits [n_paths][9]; relax_heading [n_paths] or NULL.
 *   samples_out [n_paths][sample_capacity][4] (x, y, z, heading); a path needing more samples fails.
 *   success_out [n_paths] 1/0; max_deviation_out, n_waypoints_out (after subdivision), iterations_out may be NULL.
 * Batches of requests: the arrays of a round live in one block of PINNED host memory kept by the context until it is
 * destroyed (about n_paths x sample_capacity x 32 bytes x 1.25 for the largest batch seen; ordinary memory when the runtime
 * refuses it), and the per-path host work runs on up to 16 threads from a few hundred requests on (MRS_TG_POLICY_THREADS). */
int mrs_tg_optimize_paths(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* wp_offsets, const mrs_tg_waypoint* waypoints,
                          const mrs_tg_initial_state* initial_states, const uint8_t* has_initial_state, const double* limits,
                          const uint8_t* relax_heading, const mrs_tg_policy_options* opt, int32_t sample_capacity,
                          int32_t* success_out, int32_t* n_samples_out, double* samples_out, double* max_deviation_out,
                          int32_t* n_waypoints_out, int32_t* iterations_out);

/* getWaypointInTrajectoryIdxs (src/...cpp:1461-1499) for one path; returns the number of indices written. */
int32_t mrs_tg_waypoint_trajectory_idxs(const double* samples, int32_t n_samples, const mrs_tg_waypoint* waypoints,
                                        int32_t n_waypoints, int32_t* idxs_out);

/* ---- initial condition: paths stamped in the future, before takeoff ------------------------ */

/* mrs_msgs::MpcPredictionFullState of the tracker command, already transformed into the path's frame.  Row i of each array is
 * sample i of the MPC horizon (a first step of 0.01 s, then 0.2 s steps); n_samples = 0 (arrays may be NULL): no prediction. */
typedef struct mrs_tg_prediction {
  int32_t n_samples;
  const double* position;     /* [n_samples][4] x, y, z, heading */
  const double* velocity;     /* [n_samples][4] xyz + heading_rate */
  const double* acceleration; /* [n_samples][4] xyz + heading_acceleration */
  const double* jerk;         /* [n_samples][4] xyz + heading_jerk */
} mrs_tg_prediction;

/* prepareInitialCondition (src/mrs_trajectory_generation.cpp:506-614) with the first-waypoint rule of optimize() (:650-655) for
 * one request.  Host arithmetic, no device, no context.  All times in seconds, differences the caller took from ONE clock read:
 *   tracker_pose + tracker_state: the tracker command (both NULL: none); tracker_age_s = now - its stamp (> 1.0: stale, :518);
 *   prediction: its full_state_prediction (NULL: none); uav_pose4: x, y, z, heading of the UAV state (NULL: none);
 *   path_time_offset_s = path stamp - now (0 for an unstamped path); n_path_waypoints: the request's waypoints (loop point
 *   included); dont_prepend: dont_prepend_current_state.
 * The first case that holds decides:
 *   dont_prepend                         -> no initial condition;
 *   no tracker command, or a stale one   -> the UAV state with z + takeoff_height, derivatives 0 (no UAV state: none);
 *   offset > 0.2 and k <= n_samples - 1  -> prediction row k, from the future; k = int(ceil((offset * 0.5 - 0.01) / 0.2)) + 1;
 *   otherwise                            -> the tracker command (k is still reported when offset > 0.2).
 * *drop_first_waypoint_out = offset > 0.2 and n_path_waypoints >= 2, whatever the case.  A path from the future is sampled at
 * 0.2 s and gets mrs_tg_splice_prediction after its solve.  Returns MRS_TG_OK or MRS_TG_ERR_INVALID_ARG. */
int mrs_tg_prepare_initial_condition(const mrs_tg_waypoint* tracker_pose, const mrs_tg_initial_state* tracker_state,
                                     double tracker_age_s, const mrs_tg_prediction* prediction, const double* uav_pose4,
                                     double takeoff_height, double path_time_offset_s, int32_t n_path_waypoints,
                                     int32_t dont_prepend, mrs_tg_waypoint* initial_waypoint_out,
                                     mrs_tg_initial_state* initial_state_out, int32_t* has_initial_condition_out,
                                     int32_t* from_future_out, int32_t* sample_offset_out, int32_t* drop_first_waypoint_out);

/* The pre-trajectory of a path from the future (:801-838): with k = sample_offset and k2 = int(floor((prediction_age_s - 0.01)
 * / 0.2)) + 1, where prediction_age_s = now - the stamp of the prediction held after the solve, prediction rows 0 .. k-1
 * (position + heading) are inserted in front of samples [n_samples][4] when k > k2.  Returns the spliced sample count
 * (n_samples when nothing is inserted); writes only when that fits sample_capacity.  MRS_TG_ERR_INVALID_ARG when the
 * prediction has fewer than k rows. */
int32_t mrs_tg_splice_prediction(const mrs_tg_prediction* prediction, int32_t sample_offset, double prediction_age_s,
                                 double* samples, int32_t n_samples, int32_t sample_capacity);

#ifdef __cplusplus
}
#endif
#endif /* MRS_TG_H_ */
