/* earl_physics.h -- C ABI of the batched articulated-body stepper (BASELINE config 3:
 * sawyer_door and sawyer_peg).
 *
 * STATUS: smooth dynamics, weld / joint-limit constraints, frictional contacts (spheres / points vs boxes, plate edges vs
 * capsules; friction cone per model: elliptic for the Sawyer scenes, as their MJCF asks, pyramidal for the kitchen and the minitaur -- earl_collision_model.cone,
 * DESIGN.md 16.10).  The weld's regularisers carry two factors identified on the contact-free prefixes of the reference's MuJoCo recordings (translation x 3.35,
 * rotation x 0.07: DESIGN.md 16.9; rounds 1 - 3: 4.0 and the "mocap quaternion as given" rule, section 9).  Parity with MuJoCo is UNPINNED (the
 * simulator is not available to this build): the kernel is tested against this build's own CPU reference
 * (oracle/physics_oracle.py: LinkModel) which follows MuJoCo's documented pipeline and is checked by first principles;
 * the model tables and forward kinematics ARE pinned by numbers recorded in the reference (tests/test_physics.py).
 *
 * One wavefront per env instance, per-link state staged in LDS (north_star).  Conventions as in earl_tabletop.h:
 * device pointers, caller's stream, negative error codes, no allocation, no synchronisation.
 *
 * The model is the reduced "link" form produced by tools/mjcf_compile.py (earl_benchmark_amd/models/<env>_links.npz):
 * one link per dof (the jointed body merged with its fixed descendants), parents before children.
 */
#ifndef EARL_PHYSICS_H
#define EARL_PHYSICS_H
#include <stdint.h>

#include "earl_tabletop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EARL_MAXV 16   /* links (= dofs) */
#define EARL_MAXATT 8  /* named frames attached to links (bodies / sites / geoms the env observes) */
#define EARL_MAXACT 4

typedef struct earl_link_model {
  int32_t nv, n_att, n_act, weld_att;      /* weld_att: attachment welded to the mocap body */
  int32_t n_jump;                          /* rounds of ancestor doubling the kinematics needs: ceil(log2(max depth)) */
  int32_t ball_dof;                        /* first of the three rotation dofs of the free body (always the last three dofs), -1 = none */
  int32_t nq, pad_;                        /* length of a qpos row: nv, or nv + 1 with a free body (its orientation is a unit quaternion
                                              stored at qpos[ball_dof .. ball_dof + 3], MuJoCo's layout) */
  int32_t jump[4][EARL_MAXV];              /* jump[r][l]: ancestor of link l at distance 2^r, -1 if none */
  int32_t parent[EARL_MAXV];               /* -1 = world */
  int32_t jtype[EARL_MAXV];                /* 0 hinge, 1 slide; a free joint is six links: three slides along the world axes, then
                                              2 = applies the orientation quaternion, axis = body x; 3, 3 = rigid, axes = body y, z
                                              (MuJoCo: angular velocity of a free body in body axes) */
  int32_t limited[EARL_MAXV];
  uint32_t anc_mask[EARL_MAXV];            /* bit i: link i is an ancestor of (or is) this link */
  uint32_t desc_mask[EARL_MAXV];           /* bit i: link i is in the subtree of this link (incl. itself) */
  int32_t att_link[EARL_MAXATT];           /* -1 = fixed to the world */
  int32_t act_joint[EARL_MAXACT];
  double tpos[EARL_MAXV][3], tquat[EARL_MAXV][4];   /* link frame in its parent link's frame (joint at zero) */
  double jaxis[EARL_MAXV][3], jpos[EARL_MAXV][3];
  double mass[EARL_MAXV], com[EARL_MAXV][3], inertia[EARL_MAXV][6];   /* xx yy zz xy xz yz about the COM, link axes */
  double range[EARL_MAXV][2], damping[EARL_MAXV], armature[EARL_MAXV];
  double jsolref[EARL_MAXV][2], jsolimp[EARL_MAXV][5], dof_invweight[EARL_MAXV];
  double att_pos[EARL_MAXATT][3], att_quat[EARL_MAXATT][4];
  double act_kp[EARL_MAXACT], act_ctrlrange[EARL_MAXACT][2];
  double weld_solref[2], weld_solimp[5], weld_invweight[2];
  double gravity[3], dt;
  double drag_G[EARL_MAXV], drag_b[EARL_MAXV];   /* soft velocity row per dof, cost 1/2 G (a + b v)^2: a permanent deep contact reduced at
                                                    model-compile time (the door panel standing in the table top), 0 = none */
  uint32_t cd_mask[EARL_MAXV];             /* links whose velocity enters d/dt of this link's axis: anc_mask, except that the three rotation
                                              axes of a free body all use the velocity before any of them (mj_comVel) */
} earl_link_model;

/* The same tables for models of up to 24 dofs (the kitchen: nv = 23), plus what only that model uses: dry joint
 * friction, joint springs, force-limited actuators and linear joint couplings.  A separate struct so that the 16-dof form above -- staged in LDS
 * by the Sawyer kernels, whose workgroups fill a CU's LDS to the last 200 bytes -- keeps its size.  Kernels take it when nv > EARL_MAXV. */
#define EARL_MAXV24 24
#define EARL_MAXATT24 16
#define EARL_MAXJEQ 8
#define EARL_MAXCONNECT 4
typedef struct earl_link_model24 {
  int32_t nv, n_att, n_act, weld_att;
  int32_t n_jump, ball_dof, nq, n_jeq;
  int32_t jump[5][EARL_MAXV24];
  int32_t parent[EARL_MAXV24], jtype[EARL_MAXV24], limited[EARL_MAXV24];
  uint32_t anc_mask[EARL_MAXV24], desc_mask[EARL_MAXV24];
  int32_t att_link[EARL_MAXATT24];
  int32_t act_joint[EARL_MAXACT];
  int32_t jeq_joint1[EARL_MAXJEQ], jeq_joint2[EARL_MAXJEQ];   /* coupling e: q[joint1] - c0 - c1 q[joint2] = 0 (MuJoCo <equality><joint polycoef>, linear term, qpos0 = 0) */
  double tpos[EARL_MAXV24][3], tquat[EARL_MAXV24][4];
  double jaxis[EARL_MAXV24][3], jpos[EARL_MAXV24][3];
  double mass[EARL_MAXV24], com[EARL_MAXV24][3], inertia[EARL_MAXV24][6];
  double range[EARL_MAXV24][2], damping[EARL_MAXV24], armature[EARL_MAXV24];
  double jsolref[EARL_MAXV24][2], jsolimp[EARL_MAXV24][5], dof_invweight[EARL_MAXV24];   /* every solimp of this struct (and of the collision classes used with it): power 1 or 2, or d0 == dwidth -- the
                                                                                           * nv > 16 kernels evaluate the impedance without pow() (csrc/physics_math.h imp_p2; the Python host side refuses other tables) */
  double att_pos[EARL_MAXATT24][3], att_quat[EARL_MAXATT24][4];
  double act_kp[EARL_MAXACT], act_ctrlrange[EARL_MAXACT][2];
  double weld_solref[2], weld_solimp[5], weld_invweight[2];
  double gravity[3], dt;
  double drag_G[EARL_MAXV24], drag_b[EARL_MAXV24];
  uint32_t cd_mask[EARL_MAXV24];
  double frictionloss[EARL_MAXV24];            /* dry friction: a constraint row per dof whose force is bounded by +- frictionloss (mjCNSTR_FRICTION_DOF) */
  double stiffness[EARL_MAXV24], springref[EARL_MAXV24];   /* joint spring: passive force -stiffness (q - springref) */
  double act_forcerange[EARL_MAXACT][2];       /* force-limited actuators: kp (ctrl - q) clamped to this range (+-inf: not limited) */
  double jeq_coef[EARL_MAXJEQ][2], jeq_solref[EARL_MAXJEQ][2], jeq_solimp[EARL_MAXJEQ][5], jeq_invweight[EARL_MAXJEQ];
  int32_t pair[EARL_MAXV24];                   /* the dof a coupling ties this dof to, -1 = none: dofs beyond the first tree (the arm: the first 9) are
                                                  their own trees, so without contacts the constraint Hessian is the arm's block plus 2 x 2 / 1 x 1 blocks */
  /* connect constraints (MuJoCo mjEQ_CONNECT; Bullet JOINT_POINT2POINT): the world positions of attachments con_att1[e] and con_att2[e] coincide --
   * three soft equality rows each (the minitaur's four knee closures, earl_benchmark/envs/minitaur.py:212-217).  Models with weld_att < 0 have no
   * mocap weld.  A free ROOT body (ball_dof = 3: the minitaur's base) keeps MuJoCo's qpos layout [xyz, quaternion, joints]: the qpos slot of dof
   * l > ball_dof + 2 is l + 1. */
  int32_t n_con, con_att1[EARL_MAXCONNECT], con_att2[EARL_MAXCONNECT], pad3_[3];
  double con_solref[EARL_MAXCONNECT][2], con_solimp[EARL_MAXCONNECT][5], con_invweight[EARL_MAXCONNECT];
} earl_link_model24;

/* Collision geometry of a link model: SPHERES (cylinders are chains of spheres; box corners are spheres of radius 0)
 * tested against BOXES, and EDGES (segments) tested against CAPSULES (blk_cap bit 8), over a fixed pair list; per-pair solver parameters by class (MuJoCo's geom mixing rules applied
 * at model-compile time).  At most max_con (<= EARL_MAXCON) contacts per env and timestep: the first active pairs in list order.
 * Models with nv <= 10 are limited to 8 contact slots and 16 blocks (their workgroup then fits four times into a CU's LDS). */
#define EARL_MAXSPH 96
#define EARL_MAXBOX 16
#define EARL_MAXPAIR 512
#define EARL_MAXCLS 16
#define EARL_MAXCON 12
#define EARL_MAXBLK 64     /* kernels: 16 for nv <= 10, 64 for the kitchen (nv = 23), 32 otherwise (csrc/physics.hip Lim<NV>::MB) */
typedef struct earl_collision_model {
  int32_t n_sph, n_box, n_pair, n_cls;
  /* pairs are stored box-major in blocks (one box x one set of spheres); a block is skipped when the bounding sphere of its
   * set (centre given in the frame of blk_link, -1 = world) is farther than blk_reach from the box centre */
  int32_t n_blk;
  int32_t max_con;                           /* contacts kept per env and timestep (<= EARL_MAXCON; <= 8 for models with nv <= 10): the first active pairs */
  int32_t cone;                              /* friction cone of the model's MJCF: 0 = pyramidal (four edge rows per contact), 1 = elliptic (rows normal, t1, t2 with one regulariser,
                                                MuJoCo's three-zone cost; round 4).  The kernels compile the cone per model size (csrc/physics.hip Lim<NV>::ELLIPTIC: nv <= 16, the
                                                Sawyer door and peg, metaworld_assets/scene/basic_scene.xml:2); an entry point given the other kind returns EARL_ERR_ARG
                                                (the word is copied from the device table once per device address and remembered -- not while the stream is being captured
                                                into a graph --, so a table is not to be rewritten in place with the other cone) */
  int32_t pad_;
  int32_t blk_begin[EARL_MAXBLK], blk_end[EARL_MAXBLK], blk_box[EARL_MAXBLK], blk_link[EARL_MAXBLK];
  int32_t blk_cap[EARL_MAXBLK];              /* bits 0-7: contacts a block may contribute (its first ones in pair order); the block order is the
                                                priority order of the max_con slots.  bit 8: KIND of the block, 0 = spheres / points vs a box,
                                                1 = EDGES vs a CAPSULE: the block's "box" is a capsule (axis = box z, radius = box_half[0],
                                                segment half length = box_half[2] - box_half[0]; box_half bounds it for the block's bounding
                                                test) and its "spheres" are segments (pair_rec.pos = midpoint, .dir = unit direction in the link
                                                frame, .hl = half length); test = closest points of the two segments, normal from the capsule's
                                                axis to the edge.  (A chain sphere on the flat of a plate is pushed along the plate normal; MuJoCo's
                                                box-cylinder contact pushes along the cylinder's radial direction where the plate's edge digs in.) */
  double blk_center[EARL_MAXBLK][3], blk_reach[EARL_MAXBLK];
  /* second bounding test of a block: the box of its set in the frame of blk_link (axis-aligned there; radii, edge lengths, the slack of sliding
   * members and the contact margin included) against the block's box, by the six face axes of the two boxes: a separating axis means no pair
   * of the block is within its margin, so the block is skipped.  Both tests only ever skip blocks without contacts: results do not depend on them */
  double blk_obb_center[EARL_MAXBLK][3], blk_obb_half[EARL_MAXBLK][3];
  int32_t sph_link[EARL_MAXSPH];             /* -1 = fixed to the world */
  int32_t box_link[EARL_MAXBOX];
  double sph_pos[EARL_MAXSPH][3], sph_r[EARL_MAXSPH];
  double box_pos[EARL_MAXBOX][3], box_quat[EARL_MAXBOX][4], box_half[EARL_MAXBOX][3];
  uint8_t pair_sph[EARL_MAXPAIR], pair_box[EARL_MAXPAIR], pair_cls[EARL_MAXPAIR];
  uint8_t pair_kind[EARL_MAXPAIR];           /* 0 = sphere / point vs box, 1 = edge vs capsule (= bit 8 of the block's blk_cap), 2 = CYLINDER vs box (round 5): pair_rec.pos = the cylinder's
                                                centre, .dir = its axis, .hl = half length, .r = radius, flat ends; ONE contact per pair from the box-cylinder narrow phase -- portal
                                                refinement on the two shapes inflated by half the margin each, the routine MuJoCo sends this geom pair to (its general convex
                                                collider); metaworld_assets/objects/assets/doorlockB.xml:17-20 */
  /* the same pairs, self-contained (one load per test): sphere link, class, local centre, radius, class margin */
  struct { int32_t sph_link, cls; double pos[3], r, margin, dir[3], hl; } pair_rec[EARL_MAXPAIR];
  double cls_mu[EARL_MAXCLS], cls_solref[EARL_MAXCLS][2], cls_solimp[EARL_MAXCLS][5], cls_margin[EARL_MAXCLS], cls_invw[EARL_MAXCLS];
  double cls_mu_tor[EARL_MAXCLS];            /* round 5: torsional friction coefficient [length] of a class whose contacts have condim 4 (MuJoCo: the larger condim and the elementwise larger
                                                friction of the two geoms; the Sawyer claws and pads: xyz_base.xml:163-185, friction 2 0.1 0.002); 0 = condim 3, no torsional row.
                                                Elliptic-cone models only: a fourth row per contact, the relative angular velocity about the normal scaled by mu_tor / mu */
} earl_collision_model;

/* nsub timesteps of every env.  model: DEVICE copy of an earl_link_model (nv <= 16) or of an earl_link_model24 (nv = 23); col: DEVICE copy of its earl_collision_model or
 * NULL (no contacts).  State (updated in place):
 * qpos [n, nq], qvel [n, nv]; inputs mocap_pos [n,3], mocap_quat [n,4] (used AS GIVEN in the weld's orientation rows: an unnormalised quaternion scales their residual and
 * Jacobian by its norm -- metaworld's [1, 0, 1, 0] is meant to be passed unchanged), ctrl [n, n_act];
 * att_xpos (may be NULL) [n, n_att, 3]: world positions of the attachments after the last timestep.
 * Solver start: the active-set iteration of the call's FIRST timestep starts from "every instantiated row active"; every later timestep of the same
 * call starts from the set its rows take at the previous timestep's solution (dry-friction rows always from their quadratic zone) -- MuJoCo warm-starts
 * from the previous qacc likewise.  The fixed point does not depend on the start, so one call of nsub timesteps and nsub calls of one agree whenever
 * the iteration converges within its 8 passes (always, in the door and peg soaks; 33 of 1 M kitchen timesteps did not).  The env entry points
 * (earl_sawyer_rollout, earl_kitchen_step) start every ENV step cold, so T calls of one step and one fused rollout of T run the same iteration. */
int earl_physics_step(const void* model, const earl_collision_model* col, int32_t nv, int32_t n, int32_t nsub, double* qpos, double* qvel,
                      const double* mocap_pos, const double* mocap_quat, const double* ctrl, double* att_xpos,
                      earl_stream_t stream);

/* Forward quantities of the CURRENT state without integrating (tests): qacc [n,nv], efc_force [n, 6+2nv] (may be NULL) */
int earl_physics_forward(const void* model, const earl_collision_model* col, int32_t nv, int32_t n, const double* qpos, const double* qvel,
                         const double* mocap_pos, const double* mocap_quat, const double* ctrl, double* qacc,
                         double* efc_force, double* att_xpos, earl_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Sawyer envs on the stepper.  Replaces, per env instance:
 *   SawyerXYZEnv.step [UPSTREAM metaworld, not in the reference tree; behaviour per SURVEY.md Appendix D]:
 *     mocap += clip(a[:3], -1, 1) * action_scale (float32 product), clipped to [mocap_low, mocap_high], mocap quat fixed;
 *     ctrl = [a[3], -a[3]]; frame_skip timesteps;
 *   SawyerDoorV2._get_obs          earl_benchmark/envs/sawyer_door.py:86-94   obs[14] = hand xyz, gripper opening, object xyz, goal[7]
 *   SawyerDoorV2.compute_reward    earl_benchmark/envs/sawyer_door.py:141-171 (sparse: is_successful :173-177, radius 0.02)
 *   PersistentStateWrapper.step    earl_benchmark/wrappers/persistent_state_wrapper.py:17-31  (done = steps_since_reset >= horizon)
 *   SawyerDoorV2.reset_model       earl_benchmark/envs/sawyer_door.py:111-125 (settled hand pose, object angle init + U(lo, hi))
 *   SawyerPegV2._get_obs           earl_benchmark/envs/sawyer_peg.py:134-142, _get_pos_objects :186-187 (object xyz = site pegHead)
 *   SawyerPegV2.compute_reward     earl_benchmark/envs/sawyer_peg.py:231-299 -- sparse: is_successful :301-305, radius 0.05; dense:
 *                                  metaworld's reward_utils / _gripper_caging_reward restated [UPSTREAM, unpinned]
 *   SawyerPegV2.reset_model        earl_benchmark/envs/sawyer_peg.py:192-229, get_next_goal / reset_goal :144-163
 * obs is float64 like the reference's (the demonstrations store it as float32). */
typedef struct earl_sawyer_cfg {
  int32_t n, env_offset;
  int32_t reward_type;                     /* 0 sparse, 1 dense (dense uses metaworld's tolerance(): unpinned) */
  int32_t horizon;                         /* <= 0: never done */
  int32_t frame_skip;
  int32_t att_hand, att_right, att_left, att_obj;   /* attachment indices the observation reads */
  int32_t obj_dof;                         /* dof re-initialised by reset: the door hinge, or the first of the peg's three translations */
  int32_t obj_kind;                        /* 0: hinge angle <- obj_init_angle + U(angle_noise)   (SawyerDoorV2.reset_model, sawyer_door.py:111-125)
                                              1: free body, xyz <- U(obj_low, obj_high) redrawn while its xy is within obj_reject_radius of
                                                 obj_reject_xy, orientation kept, zero velocity  (SawyerPegV2.reset_model, sawyer_peg.py:192-229)
                                              2: as 1 with probability 1/2, otherwise xyz <- wide_table[randint(n_wide)] + wide_shift +
                                                 U(-wide_noise, wide_noise)^3  (wide_init, sawyer_peg.py:200-209) */
  int32_t n_goal_rows;                     /* > 0: reset draws the goal uniformly from goal_table [n_goal_rows, 7] (SawyerPegV2.get_next_goal
                                              with reset_at_goal, sawyer_peg.py:144-152); 0: goals are left as they are */
  int32_t goal_change_frequency;           /* > 0: LifelongWrapper.step (lifelong_wrapper.py:30-44): every that many steps since the last reset /
                                              switch the goal is redrawn (from goal_table if n_goal_rows > 0, else kept) and the goal block of the
                                              observation returned by that step is the NEW goal; the reward of that step used the old one */
  int32_t n_wide;                          /* rows of wide_table (obj_kind 2) */
  int32_t att_grasp, att_lpad, att_rpad;   /* peg dense reward: site pegGrasp, bodies leftpad / rightpad (-1: sparse only) */
  int32_t pad2_;
  double action_scale;
  double mocap_low[3], mocap_high[3], mocap_quat[4];
  double success_radius;
  double hand_init_pos[3], obj_init_pos[3];
  double obj_init_angle, angle_noise[2];
  double obj_low[3], obj_high[3], obj_reject_xy[2], obj_reject_radius;
  const double* goal_table;                /* device, [n_goal_rows, 7]; may be NULL when n_goal_rows == 0 (otherwise EARL_ERR_ARG) */
  const double* wide_table;                /* device, [n_wide, 3] or NULL */
  double wide_shift[3], wide_noise;
  double init_tcp[3];                      /* peg dense reward: midpoint of the finger sites after _reset_hand (SawyerXYZEnv.init_tcp [UPSTREAM]) */
  double box_corners[4][3];                /* ... and the two keep-out prisms in front of the hole block (sites *_corner_collision_box_{1,2}, sawyer_peg.py:252-256) */
  uint64_t seed, counter;                  /* reset draws: Philox(seed; draw, global env id, counter) */
  uint64_t step_counter;                   /* env steps taken before this launch (goal-switch draws: Philox(seed; 0xFFFE, global env id, step)) */
} earl_sawyer_cfg;

typedef struct earl_sawyer_state {
  double* qpos;                 /* [n, nq] */
  double* qvel;                 /* [n, nv] */
  double* mocap_pos;            /* [n, 3] */
  double* goal;                 /* [n, 7] */
  int32_t* steps_since_reset;   /* [n] */
  int32_t* steps_since_goal_change;   /* [n]; may be NULL when cfg.goal_change_frequency == 0 (otherwise the rollout and the reset return EARL_ERR_ARG) */
  double* obj_init;             /* [n, 6] obj_init_pos, peg_head_pos_init as reset_model leaves them (sawyer_peg.py:213-215); may be NULL
                                   for sparse rewards without out.info (a peg with dense rewards or with out.info and NULL here: EARL_ERR_ARG
                                   from the rollout; with dense rewards from the reset too);
                                   written by earl_sawyer_reset, read by the peg's dense reward */
  double* last_obs;             /* [n, 14] may be NULL: the observation last returned for each env (SawyerXYZEnv._last_stable_obs [UPSTREAM]);
                                   written by earl_sawyer_reset and at the end of earl_sawyer_rollout, read when the FIRST step of a launch
                                   diverges (later steps copy the previous row of the launch's own output).  NULL and the first step diverges:
                                   that row of out.obs is NaN, and so are the rows that copy it */
  int32_t* fail_count;          /* [n] may be NULL: env steps that diverged and were rolled back (see earl_sawyer_out.status) */
  int32_t* sched;               /* may be NULL.  Scratch of the TIME-SLICED schedule of earl_sawyer_rollout: 2 * ceil(n / 4) int32, ZERO on entry (the caller clears it
                                   before every call).  When given, and the batch is larger than what the GPU holds at once (peg model: more than 16 envs per CU),
                                   the launch is a queue of (group of 4 envs, slice of 10 env steps) items taken by persistent waves, least-advanced group first,
                                   instead of one whole rollout per wave: the slow groups (envs in contact) run without a break while the fast ones share the other
                                   wave slots.  Same results (an env's arithmetic does not depend on who runs it, tests/test_sawyer_full_gpu.py); NULL = one group per wave */
} earl_sawyer_state;

typedef struct earl_sawyer_out {
  double* obs;        /* [T, n, 14] */
  float* reward;      /* [T, n] */
  uint8_t* done;      /* [T, n] */
  uint8_t* success;   /* [T, n] is_successful(obs) */
  uint8_t* status;    /* [T, n] may be NULL: 0 = ok, EARL_STEP_DIVERGED = after this env step some qpos / qvel entry was NaN or beyond
                         EARL_BAD_VALUE in magnitude (MuJoCo's mj_checkPos / mj_checkVel test with mjMAXVAL = 1e10).  Such a step is rolled
                         back: state, mocap target <- the env's last stable ones, the row carries the last stable observation, reward 0,
                         success 0 (SawyerXYZEnv.step on MujocoException [UPSTREAM]: `return self._last_stable_obs, 0.0, False, info`);
                         the step still counts for the horizon.  Other envs of the batch are unaffected. */
  double* info;       /* [T, n, EARL_SAWYER_INFO] may be NULL (no cost then): the numbers of the `info` dict the reference's step() returns through evaluate_state --
                         door earl_benchmark/envs/sawyer_door.py:127-139, peg sawyer_peg.py:165-184 -- at the EARL_INFO_* slots below.  NB the reference's
                         info['success'] is NOT is_successful(): the door uses obj_to_target <= 0.08 (is_successful: 0.02), the peg the axis-scaled distance
                         <= 0.05; and the door's 'in_place_reward' is the HAND's tolerance term (its compute_reward returns hand_in_place in that slot).
                         A rolled-back step carries zeros. */
} earl_sawyer_out;
#define EARL_SAWYER_INFO 8
#define EARL_INFO_SUCCESS 0
#define EARL_INFO_NEAR_OBJECT 1
#define EARL_INFO_GRASP_SUCCESS 2
#define EARL_INFO_GRASP_REWARD 3
#define EARL_INFO_IN_PLACE_REWARD 4
#define EARL_INFO_OBJ_TO_TARGET 5
#define EARL_INFO_UNSCALED_REWARD 6
#define EARL_BAD_VALUE 1e10
#define EARL_STEP_DIVERGED 1

/* T env steps of every env in ONE launch (state stays in LDS between steps; qpos / qvel / mocap_pos are written back after every
 * env step that ended finite -- they are the "last stable state" a diverged step rolls back to).  action: float32 [T, n, 4]. */
int earl_sawyer_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                        const float* action, int32_t T, const earl_sawyer_out* out, earl_stream_t stream);
/* As earl_sawyer_rollout, but the step-dependent Philox counters are cfg->counter + clock[0] and cfg->step_counter + clock[1], where `clock` is DEVICE memory
 * holding two uint64 that the kernel reads when it runs (NULL = zero; the rollout draws with step_counter only: clock[0] has no use here).  For launches
 * captured into a HIP graph: the captured launch of step t passes cfg->step_counter = t, and the host writes the base into the clock before each replay.
 * Every kernel the launcher picks (door default / eight-wave / 64-lane, peg) honours it; earl_sawyer_rollout is this with clock = NULL. */
int earl_sawyer_rollout_clocked(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const float* action, int32_t T, const uint64_t* clock, const earl_sawyer_out* out, earl_stream_t stream);

/* ---- closed loop: an MLP policy evaluated INSIDE the Sawyer rollout kernel ----
 * T closed-loop env steps of the door (nv = 10) or the peg (nv = 15) in ONE launch of the rollout kernel: between two env steps the 16 lanes that own an env evaluate
 * the policy, observation -> float32 MLP 14 -> hidden (-> hidden) -> 4 -> action -> next env step.  earl_mlp_policy / earl_gaussian_head are earl_tabletop.h's, with
 * dims[0] = 14 and dims[n_layers] = 4 (head = NULL) or 8 (head given: output rows 0..3 the mean, rows 4..7 the raw log_std); hidden widths multiples of 16 in 16..256;
 * policy->params 16-byte aligned (the kernel reads the weight rows in 16-byte pieces).
 * What the policy sees: at step 0 obs0 [n, 14] (device); at step t > 0 row t - 1 of THIS launch's out->obs exactly as emitted -- the repeated row of a rolled-back
 * step and the goal block patched by a lifelong goal switch included -- each double rounded to float32.
 * Arithmetic: the contract of earl_tabletop_policy_rollout (acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc); relu_f32, tanh_f32; the head's exp_f32,
 * normal_quantile_f32, log_std maps and u = fmaf(exp_f32(ls), eps, mean): csrc/policy_math.h); earl_mlp_policy_forward_cpu below states it on the host.
 * Draws of the head: ONE Philox4x32-10 block per (env, env step), key = cfg->seed, counter words {0x504F4C00, cfg->env_offset + env, ev lo, ev hi} with
 * ev = cfg->step_counter + clock[1] + t (the value the goal-switch draw of that step uses; its draw index is 0xFFFE, the reset's are 0 .. 31, 0xFFF0 .. 0xFFF2 and
 * 0xFFFF: the streams are disjoint); words x, y, z, w -> action dimensions 0 .. 3.  head->eps_out (may be NULL) is [T, n, 4] here, written in both modes.
 * actions [T, n, 4] (device, required) receives the actions as the policy produced them; the launch is bit-identical to earl_sawyer_rollout_clocked fed with it:
 * outputs, state left behind, counters.  clock as for earl_sawyer_rollout_clocked (may be NULL).
 * EARL_ERR_ARG before any HIP call: the policy and head rules of earl_tabletop.h's argument contract with the widths 14 / 4, and this entry point's own: NULL policy /
 * obs0 / actions / out->obs, policy->params not 16-byte aligned, T < 1, nv not 10 or 15, and everything earl_sawyer_rollout refuses.  The 64-lanes-per-env measurement
 * builds (earl_debug_set_physics_lanes(64)) have no policy form: EARL_ERR_ARG.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned; each widens exactly (u << 16) into the same fmaf chain, so the
 * launch returns the bits of the fp32 launch fed with the widened values. */
int earl_sawyer_policy_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_mlp_policy* policy, const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions,
                               const earl_sawyer_out* out, earl_stream_t stream);
/* ---- the same closed loop for a POPULATION of policies, with per-env episode summaries and without any [T] array ----
 * earl_policy_population / earl_episode_summary are earl_tabletop.h's, as they are.  One episode per launch: the summary rows are [n].
 *   pop      NULL = one policy: bit-identical to earl_sawyer_policy_rollout, which is this call with pop = summary = NULL.  Otherwise the env with GLOBAL id
 *            g = cfg->env_offset + i runs member g / G, whose parameters start at policy->params + (g / G) * param_stride.  The member depends on the global id only:
 *            env_offset need not be a multiple of 4, 16 or G, and a wavefront whose four envs belong to two members is correct, only slower.  The launch is
 *            bit-identical to cutting the batch at the global ids that are multiples of G and running the single-policy entry point on each piece (env_offset = its
 *            first global id, n = its length, the matching state rows) with that member's parameters: outputs, actions, eps_out, state, fail_count, counters.
 *   summary  NULL, or: ret = sum over t ascending of (double)reward_t; success_last = the success flag of step T - 1; first_success = the smallest t with success,
 *            or -1.  Each is exactly its definition applied to what out->reward / out->success hold or would hold, rolled-back rows (reward 0, success 0)
 *            included.  The env's lane 0 keeps the three words up to date in device memory after every env step (step 0 initialises them), so a time slice of
 *            the peg's schedule that another wavefront takes finds them where it finds qpos.
 *   actions and every pointer of `out`, out->obs included, may be NULL (`out` itself may not).  With out->obs == NULL the env's row of st->last_obs (then
 *            required) is the one observation row the launch keeps: every emitted row, the rollback's re-emission and the goal switch's patch are written to it, and
 *            the policy of step t + 1 reads it (lane by lane what that lane wrote; across a time slice under the release / acquire that carries qpos).  The state
 *            left behind, last_obs included, equals the full launch's.
 * EARL_ERR_ARG before any HIP call: everything earl_sawyer_policy_rollout refuses (but NULL actions / out->obs), the contract's population rules, and this entry
 * point's own: param_stride % 4 != 0 (every member's rows are read in 16-byte pieces), out->obs == NULL with st->last_obs == NULL.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_sawyer_population_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                   const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_gaussian_head* head, const double* obs0, int32_t T,
                                   const uint64_t* clock, float* actions, const earl_sawyer_out* out, const earl_episode_summary* summary, earl_stream_t stream);
/* ---- the same closed loop for the AGENT PAIR of autonomous RL: a forward and a reset agent alternating inside one rollout ----
 * earl_agent_pair is earl_tabletop.h's struct, as it is, used with these sizes: backward_goal ONE row of 7 doubles in the Sawyer goal format (as a row of st->goal);
 * agent_out [T, n]; forward_success / backward_success [n] (one launch is one episode).  policy->params is [2, param_stride]: row 0 the forward agent, row 1 the
 * reset agent, both of policy's architecture and head.  There is no EARL_PAIR_MAX_H2 limit here: the weights are read from memory at every step, not held in registers.
 * Per env and env step, in this order (the order is the contract):
 *   1. the action is computed from the observation the env last emitted (earl_sawyer_policy_rollout's rule: obs0 at step 0, row t - 1 as emitted afterwards) by the
 *      network of the env's current `phase` (0 forward, anything else reset) at policy->params + phase * param_stride; the arithmetic is unchanged;
 *   2. with a head, the step's Philox block is the one earl_sawyer_policy_rollout makes ({0x504F4C00, global id, ev}): it does not depend on the phase;
 *   3. agent_out, actions and eps_out are written;
 *   4. the env step runs as in the single-policy kernel, failure guard, rollback and fail_count included; reward and success refer to the goal in force DURING the
 *      step, which is the env's row of st->goal;
 *   5. steps_in_phase += 1 (a rolled-back step counts, with success 0), and the env hands over if (switch_on_success && success) || steps_in_phase >=
 *      switch_every[phase]: phase ^= 1, steps_in_phase = 0; forward_success / backward_success of the phase that ended is incremented if switch_on_success && success
 *      (a step where the clock ran out as well counts as ended by success); step 0 of the launch starts both counters at 0.
 *      Entering the reset phase with backward_goal != NULL, the env's row of st->goal becomes backward_goal.  Entering the forward phase with cfg->n_goal_rows > 0, it
 *      becomes the goal-table row of the lifelong switch's draw for this step (draw index 0xFFFE, global id, ev = cfg->step_counter + clock[1] + t; the same u01 and
 *      clamp); with n_goal_rows == 0 the goal stays.  Whenever the row changes, the goal block of this step's emitted observation row (out->obs, or the carried row of
 *      st->last_obs) is patched exactly as the lifelong switch patches it: the next action sees the new goal, this step's reward used the old one;
 *   6. phase and steps_in_phase are stored after every env step, so a time slice of the peg's schedule that another wavefront takes finds them, the counters and
 *      agent_out's predecessors under the release / acquire that carries qpos and the summary words.
 * Unlike the tabletop, whose goal_idx a pair launch leaves alone, st->goal IS the goal in force here and is left as such at launch exit: there is no separate entry
 * rule (an env in the reset phase starts from whatever its row of st->goal holds), and every other entry point keeps working on the state.
 * Never switching (switch_every > T, switch_on_success = 0) with all envs in phase 0 the launch is bit-identical to earl_sawyer_policy_rollout with row 0: outputs,
 * actions, eps, state, fail_count; all envs in phase 1 with backward_goal = NULL, to the same with row 1.  actions, every pointer of `out` and the pair's three output
 * pointers may be NULL, as in earl_sawyer_population_rollout; without out->obs the env's row of st->last_obs is carried.  On the door, out->info receives only what the
 * lifelong switch leaves on a goal-switch row (the door's info dict of a pair launch is not offered); the peg's is written in the kernel as ever.
 * EARL_ERR_ARG before any HIP call: everything earl_sawyer_population_rollout refuses with pop = NULL, the contract's pair rules, and this entry point's own:
 * param_stride not a multiple of 4, backward_goal != NULL with cfg->n_goal_rows == 0 (the forward goal could not be restored).
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_sawyer_pair_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                             const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_gaussian_head* head, const double* obs0, int32_t T,
                             const uint64_t* clock, float* actions, const earl_sawyer_out* out, earl_stream_t stream);
/* ---- the agent pair in its general form: a TABLE of backward goals, a POPULATION of pairs, episode SUMMARIES -- each NULL or given, in any combination ----
 * earl_sawyer_pair_rollout is this call with pop = goals = summary = NULL, bit for bit; its six items are the contract, with these additions.
 *   goals    Entering the reset phase, the env's row of st->goal becomes table[r], r = min((int)(u01(b.x, b.y) * n_rows), n_rows - 1), where b is the Philox4x32-10 block
 *            {0xFFFD, global env id, ev lo, ev hi} under key cfg->seed, ev = cfg->step_counter + clock[1] + t: the counter words, u01 and clamp of the forward entry's
 *            0xFFFE draw.  Draw index 0xFFFD is free: the reset uses 0 .. 31, 0xFFF0 .. 0xFFF2 and 0xFFFF, the goal switch 0xFFFE, the head 0x504F4C00.  The
 *            observation patch, the door's info marker and the agent-scope fence are item 5's.  goals->row[env] = r and row_out[t n + env] = r at such a step; row_out is
 *            -1 at every other step of a live env.  The draw depends on seed, global id and step only: not on n, the shard, or how the steps are cut into launches.
 *            A table of ONE row equals earl_sawyer_pair_rollout with pair->backward_goal = that row.
 *   pop      policy->params is [P, 2, pair->param_stride]: the env with GLOBAL id g runs the pair of member g / G at policy->params + (g / G) * pop->param_stride, row 0
 *            the forward agent, row 1 the reset agent.  Bit-identical to cutting the batch at the multiples of G and running earl_sawyer_pair_rollout on each piece.
 *   summary  as in earl_sawyer_population_rollout, rows [n]: each word is its definition applied to what out->reward / out->success hold or would hold -- reward and
 *            success against the goal in force DURING the step.  actions and every pointer of `out` may be NULL, as for a pair.
 * EARL_ERR_ARG before any HIP call: everything earl_sawyer_pair_rollout refuses; with pop, earl_sawyer_population_rollout's population rules and pop->param_stride <
 * 2 * pair->param_stride; goals with a NULL table or n_rows < 1, goals together with pair->backward_goal != NULL, goals with cfg->n_goal_rows == 0 (the forward goal
 * could not be restored). */
typedef struct earl_backward_goals {
  const double* table;   /* device, [n_rows, W], a row of the env's st->goal: W = 7 on the Sawyer door and peg (the Sawyer goal format), 2 on the minitaur (x, y),
                            23 on the kitchen (a qpos) */
  int32_t  n_rows;       /* >= 1 */
  int32_t  pad_;
  int32_t* row;          /* NULL or [n], caller-owned: the table row the env's reset goal came from; written at every entry into the reset phase, never read */
  int32_t* row_out;      /* NULL or [T, n]: the row drawn at env step t, -1 at a step without a draw */
} earl_backward_goals;
/* policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_sawyer_agents_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_policy_population* pop, const earl_backward_goals* goals,
                               const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_sawyer_out* out,
                               const earl_episode_summary* summary, earl_stream_t stream);

/* ---- branches: K candidate action sequences per env scored FROM THE CURRENT STATE, the state left as it is ----
 * earl_tabletop_branch_rollout's contract (earl_tabletop.h) restated for the door (nv = 10) and the peg (nv = 15): what a shooting planner (random shooting, CEM,
 * MPPI) asks of a contact-rich env -- K plans of H steps per env, one return, one success flag, one last observation and one count of rolled-back steps each,
 * nothing kept.  ONE launch of the rollout kernel over the K n virtual envs v = k n + i (branch k of env i), in front of it one small kernel that copies the env's
 * [n] state rows into the workspace's [K n]; no [H] row is written anywhere.
 *   equivalence  branch (k, i) equals earl_sawyer_rollout_clocked(model, col, nv, cfg, <a private copy of st>, act + k * act_branch_stride, H, clock, out) restricted to
 *                env i, bit for bit:  summary->ret[k n + i] = the float64 sum over t ascending of the float32 out->reward[t][i];  success_last = out->success[H - 1][i];
 *                first_success = the first t with success, or -1;  last_obs[k][i] = out->obs[H - 1][i] exactly as emitted -- the goal block a lifelong switch patched,
 *                the repeated row of a rolled-back step and, when step 0 itself diverges, the env's row of st->last_obs (NaN if that is NULL) included;
 *                fail[k n + i] = the number of steps with status == EARL_STEP_DIVERGED.  A rolled-back step restores the BRANCH's own last stable state; before its
 *                first stable step that is the state in `st`.
 *   draws        step t of EVERY branch uses ev = cfg->step_counter + clock[1] + t, and the Philox id is the env's global id cfg->env_offset + i, never the virtual
 *                index: all branches see the same lifelong goal draws (common random numbers), and each predicts what the next real rollout with those actions will do.
 *   act          float32, device.  act_branch_stride (in floats) == H * n * 4: a contiguous [K, H, n, 4] array; 0: every branch replays one [H, n, 4] block.
 *   state        `st` is read and never written: qpos, qvel, mocap_pos, goal, both step counters, obj_init, last_obs, fail_count -- and st->sched, which is not even read.
 *   ws           what the launch mutates: per virtual env the last stable qpos / qvel / mocap_pos, the goal row, the goal-switch counter and the one carried observation
 *                row (last_obs itself when given), and the work queue of the time-sliced peg form.  ONE device block: base 8-byte aligned, bytes >= what
 *                earl_sawyer_branch_ws_bytes(nv, K, n, &bytes) reports (0 for K n == 0; monotone in K and in n); the call carves it and refuses a block that is too
 *                small.  The caller prepares NOTHING in it -- the call fills every row it reads and clears the queue itself -- and nothing in it outlives the call: the
 *                same block serves any later call that fits.  No allocation, no host synchronisation: after one eager call with the same `col` (the friction-cone check
 *                reads the table's cone word once per address) the call can be captured into a HIP graph.
 *   outputs      summary (rows [K n]; the struct or any of its three pointers NULL), last_obs ([K, n, 14] or NULL) and fail ([K n] or NULL) in any combination, but not
 *                all five pointers NULL.  earl_sawyer_out.info has no counterpart here.
 *   forms        chosen by the number of VIRTUAL envs K n with earl_sawyer_rollout's rules: the door's one-wave build, its eight-wave build above 4096, the peg, and the
 *                peg's time-sliced schedule when the grid exceeds the CU count and H > 1 (the queue is the workspace's).  Those forms are held bit-identical to each
 *                other, which is what makes the equivalence above independent of K.  earl_debug_set_door_variant(3) is read as 0, as the closed loop reads it; under
 *                earl_debug_set_physics_lanes(64) the call returns EARL_ERR_ARG (the 64-lane measurement builds have no branch form).
 * EARL_ERR_ARG before any HIP call for: everything earl_sawyer_rollout_clocked refuses in model / cfg / st (goal switching without its counter, a goal count without its
 * table, peg dense reward without obj_init), nv not 10 or 15; act or ws NULL; K < 0; H < 0; a negative stride, or one that is neither 0 nor >= H * n * 4; all five outputs
 * NULL; K * n beyond 2^31 - 1; with K n > 0: ws->base NULL or misaligned, ws->bytes too small.  n == 0, K == 0 or H == 0 returns EARL_OK, launches nothing and writes
 * nothing. */
typedef struct earl_sawyer_branch_ws {
  void*   base;    /* device, 8-byte aligned; NULL-able if K n == 0 */
  int64_t bytes;   /* size of the block at `base` */
} earl_sawyer_branch_ws;
/* *bytes = the size of the workspace of a branch launch of K branches of n envs; EARL_ERR_ARG for bytes == NULL, nv not 10 or 15, K < 0, n < 0, K * n beyond 2^31 - 1 */
int earl_sawyer_branch_ws_bytes(int32_t nv, int32_t K, int32_t n, int64_t* bytes);
int earl_sawyer_branch_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                               const earl_episode_summary* summary, double* last_obs, int32_t* fail, earl_stream_t stream);

/* ---- MPPI planning on the door and the peg: I iterations of sample -> score -> reweight on the device, the env left as it is ----
 * The planner the branch launch was made for: earl_tabletop_plan_mppi's contract (earl_tabletop.h, "MPPI planning", items 1 - 7) with FOUR action dimensions.  Unlike
 * the tabletop's, the candidates go THROUGH MEMORY: an env step here costs tens of thousands of cycles and the whole [K, H, n, 4] array of a realistic call is about a
 * megabyte, so the scoring launch is earl_sawyer_branch_rollout itself, untouched, between two small kernels.  Per iteration on the caller's stream: the candidates
 * kernel, earl_sawyer_branch_rollout (its replicate kernel and its rollout kernel), the update kernel; no allocation, no host synchronisation: after one eager call
 * with the same `col` (the branch launch's rule) the call can be captured into a HIP graph.  noise_counter is a host word: a captured call replays the same noise.
 * For iteration j = iteration0 + i (i = 0 .. iterations - 1), env `env` with global id g = cfg->env_offset + env, and the plan entering the iteration `mean` (the
 * argument for i = 0, the previous iteration's result afterwards):
 *   1 clipped mean  m[t][d] = clip(mean[t][d]) in float32 for d = 0 .. 3, clip(x) = (y = x > -1 ? x : -1; y < 1 ? y : 1) = min(max(x, -1), 1).  ALL FOUR dimensions are
 *                   clipped, the gripper word included; the rollout kernel itself clips only x, y, z (set_xyz_action) and takes the gripper word as given.
 *   2 candidates    branch 0 is the plan itself, a_0 = m.  For k >= 1: a_k[t][d] = clip(fmaf(sigma[d], eps_d, m[t][d])), eps_d = normal_quantile_f32(word_d >> 8)
 *                   (csrc/policy_math.h; earl_normal_quantile_f32), words x, y, z, w of ONE Philox4x32-10 block serving d = 0, 1, 2, 3: key = cfg->seed, counter
 *                   words = {0x504C4E00 | j, g, (k << 16) | t, noise_counter}.  Word 0 collides with no other draw of the Sawyer envs (they use 0 .. 31, 0xFFF0 .. 0xFFF2
 *                   and 0xFFFD .. 0xFFFF, the Gaussian head 0x504F4C00).  The draws depend on (seed, g, j, k, t, noise_counter) only: not on n, not on the shard split.
 *   3 scores        ret[k][env] = summary->ret of earl_sawyer_branch_rollout fed with those candidates (act_branch_stride = H * n * 4) and the caller's `clock`: goal
 *                   switches inside the look-ahead and rolled-back steps (reward 0) count exactly as that call defines them.  The metaworld rewards are
 *                   non-negative, so a rolled-back step never scores above an honest one.
 *   4 weights       beta = max_k ret[k];  x_k = (float)((ret[k] - beta) * inv_temperature) (two float64 roundings);  w_k = exp_f32(x_k) (csrc/policy_math.h;
 *                   earl_exp_f32);  W_k = (double)w_k * 2^24 rounded to nearest-even as int64 (0 .. 2^24);  S = sum_k W_k (>= 2^24: the best branch has W = 2^24).
 *   5 update        delta = a_k[t][d] - m[t][d] (one float32 subtraction);  D_k = (double)delta * 2^20 rounded to nearest-even as int64;  A = sum_k W_k * D_k in
 *                   int64 (|A| < 2^59 for K <= 8192);  mean'[t][d] = clip(m[t][d] + (float)((double)A / ((double)S * 2^20))), (double)A rounded to nearest.
 *                   Integer sums are associative: the result does not depend on how the K branches are spread over lanes, waves and workgroups.
 *   6 outputs       plan [H, n, 4] float32, REQUIRED: the mean after the last iteration; it may be the pointer `mean` itself (the in-place call), any other overlap of
 *                   the two arrays is refused.  ret [K, n] float64, REQUIRED: the last iteration's returns on exit.  ret0 NULL or [iterations, n] float64: the
 *                   return of the plan entering each iteration (branch 0).  best_ret NULL or [n] float64: beta of the last iteration.  best_k NULL or [n] int32:
 *                   the smallest k attaining it (earl_sawyer_plan_candidates recovers that candidate).  fail NULL or [K, n] int32: the last iteration's count of
 *                   rolled-back steps per branch (earl_sawyer_branch_rollout's `fail`).
 *   7 non-finite    clip() maps a NaN of `mean` to -1 and +-Inf to +-1, so every candidate is finite whatever `mean` holds.  A NaN return never wins: beta is the
 *                   largest return that is not NaN, -Inf if there is none; x_k that is NaN (a NaN return, or Inf - Inf) gives W_k = 0; if S == 0 (no branch has a
 *                   weight) the update is skipped, mean' = m.  best_k is the smallest k with ret[k] == beta when beta > -Inf, and 0 otherwise.  Nothing of this faults.
 *   chaining        `iterations` iterations in one call equal that many calls with iterations = 1 and iteration0 = j, each fed the previous plan, bit for bit.
 *   state           `st` is read and never written, as in the branch launch: the env is as earl_sawyer_branch_rollout leaves it.
 *   ws              ONE block as earl_sawyer_branch_ws describes it, of at least earl_sawyer_plan_ws_bytes(nv, K, H, n, &bytes) bytes: the branch launch's workspace
 *                   and behind it the [K, H, n, 4] candidates of the current iteration (the call aligns them to 16 bytes itself).  The size is monotone in K, H
 *                   and n and 0 for K n == 0.  The caller prepares nothing in it and nothing in it outlives the call.
 * EARL_ERR_ARG before any HIP call for: everything earl_sawyer_branch_rollout refuses in model / col / cfg / st / nv; params, mean, plan, ret or ws NULL; K outside
 * 1 .. EARL_SAWYER_PLAN_MAX_K (one env's integer weights are held in 32 KB of LDS); H outside 1 .. 65536; iterations < 1, iteration0 < 0, iteration0 + iterations > 256;
 * a sigma that is negative or not finite; an inv_temperature that is not finite or <= 0; plan overlapping mean without being equal to it; K * n beyond 2^31 - 1; with
 * n > 0 a ws block that is NULL, misaligned (8 bytes) or too small.  n == 0 returns EARL_OK, launches nothing and writes nothing.  Under
 * earl_debug_set_physics_lanes(64) the call returns EARL_ERR_ARG, as the branch launch does. */
typedef struct earl_sawyer_plan_params {
  int32_t K;               /* candidates per env, branch 0 (the plan itself) included: 1 .. EARL_SAWYER_PLAN_MAX_K */
  int32_t H;               /* steps of a plan: 1 .. 65536 */
  int32_t iterations;      /* I >= 1 */
  int32_t iteration0;      /* index of the first iteration (a word of the noise counter): >= 0, iteration0 + iterations <= 256 */
  float sigma[4];          /* noise scale per action dimension (x, y, z, gripper), finite, >= 0 */
  uint32_t noise_counter;  /* a word of the noise counter: a fresh value per control step gives fresh noise */
  double inv_temperature;  /* 1 / lambda, finite, > 0 */
} earl_sawyer_plan_params;
#define EARL_SAWYER_PLAN_MAX_K 8192
/* *bytes = the size of the workspace of a planner call; EARL_ERR_ARG for bytes == NULL, nv not 10 or 15, K < 0, H < 0, n < 0, K * n beyond 2^31 - 1 */
int earl_sawyer_plan_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes);
int earl_sawyer_plan_mppi(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                          const earl_sawyer_plan_params* params, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                          int32_t* fail, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream);
/* Item 2 written out for ONE iteration j (0 .. 255): act_out [K, H, n, 4] float32, 16-byte aligned, what earl_sawyer_branch_rollout takes; earl_sawyer_plan_mppi runs
 * the same kernel.  It reads cfg->n, env_offset and seed and params->K, H, sigma and noise_counter only (no env state, no model: one entry point serves both envs).
 * EARL_ERR_ARG for cfg, params, mean or act_out NULL, act_out misaligned, n < 0, K or H out of range, j outside 0 .. 255, a bad sigma, K * n beyond 2^31 - 1; n == 0
 * returns EARL_OK and writes nothing. */
int earl_sawyer_plan_candidates(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream);
/* Host twins of the planner's own arithmetic (libearl_host.so; host pointers; csrc/sawyer_plan.h in plain loops -- there is no host stepper, so the scores are the
 * caller's).  earl_sawyer_plan_candidates_cpu: the call above (no alignment asked of act_out).  earl_sawyer_plan_update_cpu: items 4 - 7 of iteration j on GIVEN
 * candidates act [K, H, n, 4] and returns ret [K, n] -> plan [H, n, 4] (may be `mean`), and ret0_row / best_ret / best_k, each NULL or [n].  It reads cfg->n and
 * params->K, H and inv_temperature; its refusals are the planner's for those, for j and for the pointers. */
int32_t earl_sawyer_plan_candidates_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, float* act_out);
int32_t earl_sawyer_plan_update_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, const float* act, const double* ret,
                                    float* plan, double* ret0_row, double* best_ret, int32_t* best_k);

/* ---- CEM planning on the door and the peg: elites instead of weights, a refitted std per (step, env, dim), the elite set found in O(K) ----
 * earl_tabletop_plan_cem's contract (earl_tabletop.h, "CEM planning", items 1 - 7) with FOUR action dimensions, around the same three launches per iteration as
 * earl_sawyer_plan_mppi: a candidates kernel, earl_sawyer_branch_rollout untouched and through the public ABI, an update kernel.  The candidates go through memory,
 * as MPPI's do here, so the update READS the elites back instead of regenerating them.  For iteration j = iteration0 + i, env with global id g = cfg->env_offset +
 * env, the entering plan `mean` and the entering std (`std0` for i = 0, the previous iteration's results afterwards):
 *   1 clipped mean and clamped std   m = clip(mean) on all four words, as MPPI item 1 above.  s = sclamp(std) per word, sclamp(x) = (y = x > std_min ? x : std_min;
 *                   y < std_max ? y : std_max): a NaN maps to std_min.  With std0 == NULL every row's std is sclamp(sigma[d]).
 *   2 candidates    branch 0 is m.  For k >= 1: a_k[t][d] = clip(fmaf(s[t][d], eps_d, m[t][d])), eps_d = normal_quantile_f32(word_d >> 8), words x, y, z, w of ONE
 *                   Philox4x32-10 block serving d = 0 .. 3: key = cfg->seed, counter words = {0x43454D00 | j, g, (k << 16) | t, noise_counter}.  Word 0 collides with
 *                   no other draw of the Sawyer envs: checked against the list of MPPI item 2 above -- they use 0 .. 31, 0xFFF0 .. 0xFFF2 and 0xFFFD .. 0xFFFF, the
 *                   Gaussian head 0x504F4C00 and MPPI 0x504C4E00 .. 0x504C4EFF; 0x43454D00 .. 0x43454DFF meets none of these.
 *   3 scores        ret[k][env] = summary->ret of earl_sawyer_branch_rollout fed with those candidates, exactly as earl_sawyer_plan_mppi calls it (act_branch_stride =
 *                   H * n * 4, the caller's `clock`, `fail` of the last iteration).
 *   4 elites        a total order over the K branches: k stands before k' iff ret[k] is not NaN and ret[k'] is NaN; or neither is NaN and ret[k] > ret[k']; or
 *                   (ret[k] == ret[k'], or both are NaN) and k < k'.  rank_k = the number of branches before k.  k is an elite iff rank_k < E and ret[k] is not NaN;
 *                   Ne = the number of elites.  The elite set is defined by this order and by nothing in the implementation (which is a radix select over the
 *                   order's 64-bit keys: linear in K).  best_ret and best_k: MPPI items 6, 7.
 *   5 update        per (t, d), over the elites in any order, every sum integer: D_k = rint((double)(a_k - m) * 2^20) as int64, a_k READ from the candidates (the
 *                   subtraction one float32 operation; branch 0 has D = 0).  A1 = sum D_k, A2 = sum D_k^2, V = Ne * A2 - A1^2.  e_mean = m + (float)((double)A1 /
 *                   ((double)Ne * 2^20)).  e_std = sqrtf((float)((double)V / ((double)Ne * (double)Ne * 2^40))), the float32 square root, correctly rounded.
 *                   mean' = clip(fmaf(alpha, m - e_mean, e_mean)); std' = sclamp(fmaf(alpha, s - e_std, e_std)).  Ne == 0 (every return NaN): mean' = m, std' = s.
 *                   Bounds: a_k and m lie in [-1, 1], so |D_k| <= 2^21 and D_k^2 <= 2^42; A2 <= Ne * 2^42 and |A1| <= Ne * 2^21.  Ne * A2 <= Ne^2 * 2^42 and
 *                   A1^2 <= Ne^2 * 2^42 stay <= 2^62, exact in int64, only for Ne <= 2^10.  Hence elites is in 1 .. min(K, EARL_SAWYER_CEM_MAX_E) with
 *                   EARL_SAWYER_CEM_MAX_E = 1024, while K itself goes to EARL_SAWYER_PLAN_MAX_K = 8192 (V >= 0 by Cauchy-Schwarz).
 *   6 outputs       plan [H, n, 4]: may be `mean` itself.  std [H, n, 4], REQUIRED: the workspace between iterations and a result; may be `std0` itself.  Any other
 *                   overlap among the four arrays is refused.  ret [K, n], REQUIRED.  ret0, best_ret, best_k, fail: as MPPI.  elite NULL or [K, n] uint8: 1 where
 *                   branch k is an elite of the LAST iteration, 0 elsewhere.
 *   7 chaining, state, non-finite   as MPPI: I iterations in one call equal I calls of one, each fed the previous plan and std; `st` is never written; nothing
 *                   faults on NaN or Inf in mean, std0 or the state; a NaN return is never an elite.
 *   ws              a block of earl_sawyer_plan_ws_bytes(nv, K, H, n, &bytes) bytes, the layout earl_sawyer_plan_mppi carves: there is no size function of its own.
 * EARL_ERR_ARG before any HIP call for: everything earl_sawyer_plan_mppi refuses (there is no temperature); elites outside 1 .. min(K, EARL_SAWYER_CEM_MAX_E); an alpha
 * that is not finite or outside [0, 1); std_min / std_max not finite or not 0 <= std_min <= std_max; std NULL; the overlaps of item 6; an act, act_out, plan or std that is
 * not 16-byte aligned (a row is one 16-byte access; the host twins ask no alignment).  n == 0 returns EARL_OK and writes nothing.
 * earl_sawyer_cem_candidates: item 2 written out for ONE iteration j (0 .. 255), act_out [K, H, n, 4], 16-byte aligned; std NULL: sigma.  It reads cfg->n, env_offset
 * and seed and params->K, H, sigma, noise_counter, std_min and std_max only.
 * earl_sawyer_cem_update: items 4 - 7 of iteration j on GIVEN device candidates act [K, H, n, 4] (16-byte aligned, every word in [-1, 1]) and returns ret [K, n]:
 * the launch earl_sawyer_plan_cem itself makes after the branch launch, public so that the selection can be driven with crafted returns without stepping physics.
 * std_in NULL: sigma.  plan may be `mean`, std may be `std_in`; ret0_row, best_ret, best_k ([n]) and elite ([K, n]) may each be NULL.  It reads cfg->n and params->K, H,
 * elites, sigma, alpha, std_min and std_max. */
#define EARL_SAWYER_CEM_MAX_E 1024
typedef struct earl_sawyer_cem_params {
  int32_t K, H, iterations, iteration0;   /* as earl_sawyer_plan_params; K in 1 .. EARL_SAWYER_PLAN_MAX_K */
  int32_t elites;                          /* E: 1 .. min(K, EARL_SAWYER_CEM_MAX_E) */
  float sigma[4];                          /* the std of every row when no std0 is given; finite, >= 0 */
  uint32_t noise_counter;
  float alpha;                             /* smoothing: finite, 0 <= alpha < 1 */
  float std_min, std_max;                  /* finite, 0 <= std_min <= std_max */
} earl_sawyer_cem_params;
int earl_sawyer_plan_cem(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                         const earl_sawyer_cem_params* params, const float* mean, const float* std0, float* plan, float* std, double* ret, double* ret0,
                         double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream);
int earl_sawyer_cem_candidates(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out,
                               earl_stream_t stream);
int earl_sawyer_cem_update(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std_in, const float* act,
                           const double* ret, float* plan, float* std, double* ret0_row, double* best_ret, int32_t* best_k, uint8_t* elite, earl_stream_t stream);
/* Host twins (libearl_host.so; host pointers, no alignment asked): csrc/sawyer_cem.h in plain loops, the elites by a sort under the order of item 4. */
int32_t earl_sawyer_cem_candidates_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out);
int32_t earl_sawyer_cem_update_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std_in, const float* act,
                                   const double* ret, float* plan, float* std, double* ret0_row, double* best_ret, int32_t* best_k, uint8_t* elite);

/* ---- discount and a terminal value on the door and the peg: the branch launch and both planners with ret = sum_t gamma^t r_t + gamma^H V(o_H) ----
 * Under the sparse reward the plain H-step sum is blind whenever the goal is more than H steps away (earl_tabletop.h, "discounted MPPI with a terminal value"); an env
 * step here costs tens of thousands of cycles, so H stays short and the remedy matters more than on the tabletop.  Both parts travel in the tabletop's struct
 * earl_plan_value.  For virtual env v = k n + i, with r_t, the rolled-back rule, success, first_success, fail and last_obs exactly as earl_sawyer_branch_rollout
 * defines them:
 *   discount   d_0 = 1.0, ret = 0.0; for t ascending: term = d_t * (double)r_t; ret = ret + term; d_{t+1} = d_t * gamma -- three float64 roundings per step, no fused
 *              multiply-add (value_accumulate of csrc/tabletop_value.h).  A rolled-back step contributes r = 0 and still advances d.
 *   terminal   ret = ret + d_H * (double)V(o_H), two float64 roundings.  o_H is the branch's last observation row exactly as `last_obs` returns it -- the patched goal
 *              block of a goal switch, the repeated row of a rolled-back step, the env's own row of st->last_obs when step 0 diverges (NaN without one) --, each
 *              double rounded to float32 as the closed-loop policy reads its rows.  V is evaluated under the policy contract (csrc/policy_math.h: acc = b_j; k ascending:
 *              acc = fmaf(x_k, W_jk, acc); relu_f32 / tanh_f32, out_act last); earl_mlp_policy_forward_cpu with a 1-wide last layer and head = NULL states it on the host.
 *              A row that holds a NaN gives ret = NaN whatever the network (relu_f32 would map a NaN pre-activation to 0 and hide it): the planners' "a NaN return
 *              never wins" rules (MPPI item 7, CEM item 4) then apply unchanged.
 *   network    pv->value: 14 -> hidden (-> hidden) -> 1, float32 (precision 0), no Gaussian head, hidden widths multiples of 16 up to 256 (the closed loop's
 *              kPolicyMaxWidth: the 16 lanes of a virtual env evaluate it after the look-ahead, nothing is held in one lane's registers, so the tabletop's
 *              EARL_PLAN_VALUE_MAX_H1 does not apply), params 16-byte aligned.  NULL: no terminal term.  With a network summary->ret is required.
 *   identity   pv == NULL or {1.0, NULL}: the call IS the value-free entry point (it forwards; the workspace may then be that entry point's).  discount == 1.0 with a
 *              network: the unchanged branch kernels followed by the value kernel, ret == plain ret + (double)V exactly.  Only discount != 1.0 reaches the rollout
 *              kernel's discounted build (the same kernel text: csrc/physics_branch_value.hip, physics_branch_value_w8.hip), in all four launch forms; d_t travels
 *              through [K n] words of the workspace beside ret, because nothing of a branch lives across a timestep and a time slice may be another wave's.
 *   planners   earl_sawyer_plan_mppi_value / earl_sawyer_plan_cem_value: earl_sawyer_plan_mppi / earl_sawyer_plan_cem with item 3 ("scores") replaced by
 *              earl_sawyer_branch_rollout_value and nothing else changed -- candidates, weights, elites, integer moments, chaining, non-finite rules, outputs.
 *   ws         ONE size function for the three calls: earl_sawyer_value_ws_bytes(nv, K, H, n, &bytes) >= earl_sawyer_plan_ws_bytes(nv, K, H, n); H = 0 is what
 *              earl_sawyer_branch_rollout_value needs (the branch launch's block and the [K n] discounts), H > 0 adds a planner's candidates.  Monotone in K, H and n,
 *              0 for K n == 0.  No allocation and no host synchronisation; capture into a graph under the branch launch's rule.
 * EARL_ERR_ARG before any HIP call for: everything the value-free entry point refuses; a discount that is NaN, <= 0 or > 1; a value network the rules above refuse
 * (widths, a precision other than 0, the activation enums, dims[3] != 0 with one hidden layer, params NULL or misaligned); a network without summary->ret; a ws block
 * that is NULL, misaligned or smaller than earl_sawyer_value_ws_bytes says.  There is no bf16 value network and no fused control loop on these
 * envs (policy-prior branches: the next section); the minitaur has the plain MPPI planner only (earl_minitaur_plan_mppi), the kitchen has none.
 * Host twin (libearl_host.so; host pointers): earl_sawyer_value_terminal_cpu adds the terminal term to ret [rows] for given last_obs [rows, 14] -- d_H by the recurrence,
 * the float32 rounding, the NaN rule and the two roundings through csrc/sawyer_value.h, the header the kernel uses; V by earl_mlp_policy_forward_cpu's loops.  pv->value
 * NULL leaves ret as it is.  There is no host stepper, so the discounted sum itself has no twin.  Its refusals: pv, last_obs or ret NULL, rows < 0, H < 0, and pv's. */
int earl_sawyer_value_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes);
int earl_sawyer_branch_rollout_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                     int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_plan_value* pv,
                                     const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary, double* last_obs, int32_t* fail, earl_stream_t stream);
int earl_sawyer_plan_mppi_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const earl_sawyer_plan_params* params, const earl_plan_value* pv, const float* mean, float* plan, double* ret, double* ret0,
                                double* best_ret, int32_t* best_k, int32_t* fail, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream);
int earl_sawyer_plan_cem_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_sawyer_cem_params* params, const earl_plan_value* pv, const float* mean, const float* std0, float* plan, float* std, double* ret,
                               double* ret0, double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                               earl_stream_t stream);
int32_t earl_sawyer_value_terminal_cpu(const earl_plan_value* pv, int32_t H, int32_t rows, const double* last_obs, double* ret);

/* ---- policy-prior branches on the door and the peg: some of the K candidates are closed-loop rollouts under a learned policy ----
 * The rewards here are sparse or contact-gated and K is small (an env step costs tens of thousands of cycles): zero-mean noise around a zero plan almost never reaches
 * the handle or the peg, a learned forward agent does.  P of the K branches of a call are therefore driven by a policy that sees the branch's own observations.
 *   placement  the prior branches are the LAST P: k = K - P .. K - 1.  (The tabletop's earl_tabletop_plan_prior uses 1 .. P; here the tail makes "the plain launch over the
 *              first (K - P) n virtual envs, the prior launch over the rest" two contiguous ranges of v = k n + i.)  Branch 0 stays the plan itself; CEM's tie order
 *              (k ascending) therefore prefers the plan and the noise branches over the prior on exact ties, and so does MPPI's best_k.
 *   action     of prior branch k at step t of env i (global id g): x_t = the float32 rounding of the row the branch last emitted, exactly as it stands -- a rolled-back
 *              step's repeated row, the goal block a lifelong switch patched -- and at t = 0 obs0[i]; u = the policy contract's output (csrc/policy_math.h;
 *              earl_mlp_policy_forward_cpu states it on the host); a[t][d] = clip(fmaf(sigma[d], eps_d, u[d])) with eps_d from the SAME Philox block noise branch k
 *              would have drawn for (j, g, k, t, noise_counter) (planner item 2: words x, y, z, w for d = 0 .. 3; word 0 is the calling planner's -- MPPI's for
 *              earl_sawyer_branch_rollout_prior) and the planner's clip on all four words.  The row is stored into the branch's block of the [K, H, n, 4] array the call
 *              scores, and into prior->act when given.  Everything else about the branch is the branch launch's contract: draws, rollback, summary, fail, common
 *              random numbers over branches.
 *   calls      earl_sawyer_branch_rollout_prior: earl_sawyer_branch_rollout_value with `act` float* [K, H, n, 4] -- the blocks of the first K - P branches are inputs,
 *              the last P blocks outputs; a stride of 0 is refused when P > 0 -- and the iteration j (0 .. 255) and noise_counter of the noise words.
 *              earl_sawyer_plan_mppi_prior / earl_sawyer_plan_cem_prior: the `_value` planners with item 3 replaced by that call: the candidates kernel still writes
 *              the tail rows, the prior launch overwrites them, in every iteration with that iteration's noise word; the update kernels read the candidates back
 *              and do not change, so `chaining` holds as it stands.  pv NULL: undiscounted, no network.
 *   launches   P > 0: ONE launch of the prior kernel (csrc/physics_branch_prior.hip, physics_branch_prior_w8.hip: the rollout kernel's fourth inclusion, built with the
 *              discounted sum only -- gamma == 1 gives the plain sum's bits) over all K n virtual envs behind the one replicate launch; the branches in front of K - P
 *              load their action inside it as a plain branch does, and a wave that holds no prior branch never enters the policy phase.  The other shape -- the
 *              untouched branch kernels over the first (K - P) n virtual envs, then the prior kernel over the last P n, each behind a replicate launch of its own and in
 *              the form its own count of virtual envs selects -- is kept behind earl_debug_set_sawyer_prior_launches(2); it measured 1.5 - 1.9 x slower where K n fits
 *              one round of waves.  The shapes and the forms are bit-identical.  Either way everything runs on the caller's stream: no second stream, no
 *              event, capturable without parallel graph branches.
 *   identities branches == 0 makes exactly the launches of the `_value` call (of the plain call when pv is NULL or {1.0, NULL}): the same bits.  After a call, feeding
 *              the full [K, H, n, 4] array to earl_sawyer_branch_rollout[_value] reproduces every output of every branch bit for bit (the replay identity).
 *   ws         earl_sawyer_prior_ws_bytes(nv, K, H, n, &bytes) >= earl_sawyer_value_ws_bytes(nv, K, H, n) for the three calls (H = 0: the branch call's own): the
 *              `_value` block with a second work queue of 8 ceil(K n / 4) bytes (rounded up to 8) behind the [K n] discounts -- the time-sliced peg queue is per
 *              launch, and the two-launch shape needs one for each -- and, H > 0, the candidates behind that.  Monotone in K, H and n, 0 for K n == 0.
 * EARL_ERR_ARG before any HIP call for: everything the `_value` call refuses; prior or prior->policy NULL; branches outside 0 .. K - 1; a policy that is not
 * 14 -> hidden (-> hidden) -> 4 with hidden widths multiples of 16 up to 256, float32 (precision 0: no bf16 prior), params 16-byte aligned, no Gaussian head, one network;
 * a sigma that is not finite and >= 0; and with P > 0: obs0 NULL, a stride of 0, `act` or prior->act not 16-byte aligned, a stride that is no multiple of 4, K above
 * EARL_SAWYER_PLAN_MAX_K or H above 65536 (the noise key), j outside 0 .. 255, prior->act overlapping an input (the candidates / mean / std0, obs0, the parameters);
 * under earl_debug_set_physics_lanes(64) as the branch launch.
 * Host twin (libearl_host.so; host pointers): earl_sawyer_prior_actions_cpu computes the [H, n, 4] action rows of prior branch k for GIVEN observation rows [H, n, 14]
 * (row (t, i) = what the branch saw at step t), with earl_mlp_policy_forward_cpu's loops and the planner's noise function (csrc/sawyer_plan.h); cem != 0 takes CEM's
 * draw word.  There is no host stepper, so that is all a twin can state.  prior->obs0 and prior->act are not read. */
typedef struct earl_sawyer_plan_prior {
  const earl_mlp_policy* policy;  /* 14 -> H1 (-> H2) -> 4, float32, no Gaussian head, one network (no population) */
  int32_t branches;               /* P: 0 .. K - 1 */
  float sigma[4];                 /* finite, >= 0 */
  const double* obs0;             /* [n, 14] device: what the policy sees at step 0 (as earl_sawyer_population_rollout's obs0) */
  float* act;                     /* NULL or [P, H, n, 4]: the prior branches' actions of the last iteration */
} earl_sawyer_plan_prior;
int earl_sawyer_prior_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes);
int earl_sawyer_branch_rollout_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                     int32_t K, int32_t H, float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_plan_value* pv,
                                     const earl_sawyer_plan_prior* prior, int32_t j, uint32_t noise_counter, const earl_sawyer_branch_ws* ws,
                                     const earl_episode_summary* summary, double* last_obs, int32_t* fail, earl_stream_t stream);
int earl_sawyer_plan_mppi_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const earl_sawyer_plan_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, float* plan,
                                double* ret, double* ret0, double* best_ret, int32_t* best_k, int32_t* fail, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                                earl_stream_t stream);
int earl_sawyer_plan_cem_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_sawyer_cem_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, const float* std0,
                               float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail, const uint64_t* clock,
                               const earl_sawyer_branch_ws* ws, earl_stream_t stream);
int32_t earl_sawyer_prior_actions_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_prior* prior, int32_t H, int32_t k, int32_t j, uint32_t noise_counter, int32_t cem,
                                      const double* obs, float* act);

/* The policy contract on the host (libearl_host.so; host pointers): actions [n, A] of n observation rows obs [n, dims[0]], dims[0] in 1..256, hidden widths in 1..256,
 * the last layer A wide (head = NULL) or 2 A wide (rows 0..A-1 the mean, A..2A-1 the raw log_std), A >= 1.  eps [n, A] = the standard-normal draws to use with a
 * head in EARL_HEAD_SAMPLE mode; NULL (or EARL_HEAD_MEAN, or no head) evaluates the mean / the deterministic policy.  policy->out_act is applied last, as on the
 * device.  The oracle of the in-kernel policies' actions; EARL_OK or EARL_ERR_ARG.  (Not the `_cpu` twin of a device entry point: there is none.)
 * policy->precision == EARL_PRECISION_BF16: params holds uint16_t bf16 values (16-byte aligned), each widened exactly (u << 16) before it enters the chain -- the host
 * statement of the stepper envs' bf16 launches, equal bit for bit to this call with precision = 0 on the widened values. */
int32_t earl_mlp_policy_forward_cpu(const earl_mlp_policy* policy, const earl_gaussian_head* head, int32_t n, const float* obs, const float* eps, float* actions);
/* the contract's scalar functions as compiled into libearl_host.so (csrc/policy_math.h): tanh_f32, exp_f32 and normal_quantile_f32 of a 24-bit k = word >> 8 */
float earl_tanh_f32(float x);
float earl_exp_f32(float x);
float earl_normal_quantile_f32(uint32_t k24);

/* reset the envs with mask[i] != 0 (mask NULL = all): state <- the settled post-_reset_hand state (reset_qpos [nq], reset_qvel
 * [nv], device), object re-initialised as cfg.obj_kind says, mocap <- hand_init_pos, counters cleared; obs [n,14]
 * (may be NULL: the state, st.obj_init and st.last_obs are still written) is written for the reset envs only. */
int earl_sawyer_reset(const earl_link_model* model, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                      const double* reset_qpos, const double* reset_qvel, const uint8_t* mask, double* obs,
                      earl_stream_t stream);

/* obs [n,14] of the CURRENT state (kinematics recomputed, nothing integrated): SawyerDoorV2._get_obs sawyer_door.py:86-94 */
int earl_sawyer_observe(const earl_link_model* model, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                        double* obs, earl_stream_t stream);

/* compute_reward / is_successful on caller-supplied observations [n,14] (sawyer_door.py:141-177); reward / success may be NULL.
 * With reward_type sparse this is also SawyerPegV2's rule (sawyer_peg.py:295-305: radius 0.05 in cfg.success_radius). */
int earl_sawyer_door_reward(const earl_sawyer_cfg* cfg, int32_t n, const double* obs, float* reward, uint8_t* success,
                            earl_stream_t stream);
/* the info dict of SawyerDoorV2.step (evaluate_state, earl_benchmark/envs/sawyer_door.py:127-139) for n observation rows [n, 14] -> info [n, EARL_SAWYER_INFO]
 * (slots EARL_INFO_*); every entry is a function of the observation and the reward type.  status (may be NULL): rows of rolled-back steps get zeros.
 * With cfg->goal_change_frequency > 0 -- and only then -- info[.][7] is also an INPUT: 1.0 marks a row whose slots 0-2 hold the target to evaluate against instead of
 * the row's own goal block.  earl_sawyer_rollout (nv = 10, goal switching on, out->info given) writes that slot for EVERY row it emits: 1.0 and the old target on
 * goal-switch rows -- the reward of such a row was computed with the goal in force BEFORE the switch (wrappers/lifelong_wrapper.py:30-44: step(), i.e.
 * evaluate_state, then reset_goal), while its observation already carries the new goal --, 0.0 on all others; the caller prepares nothing.  Without goal switching
 * the slot is output only (whatever the buffer held is ignored).
 * (The peg's dict needs simulator state -- the pegGrasp site, the pads: earl_sawyer_out.info of earl_sawyer_rollout carries it.) */
int earl_sawyer_door_info(const earl_sawyer_cfg* cfg, int32_t n, const double* obs, const uint8_t* status, double* info, earl_stream_t stream);

/* measurement switch: lanes of a wavefront that work on one env instance -- 16 (default: four envs per wavefront) or 64 (one
 * wavefront per env).  Results are identical; DESIGN.md quotes both timings. */
/* The entry points that take a collision table check its friction cone against the kernels' (earl_collision_model.cone) by reading the cone word of the DEVICE table
 * once per address and remembering it.  The owner of a table must announce that its block is freed or rewritten -- a caching allocator hands the same address to the
 * next table, which may be of the other cone: col = the table's device address, or NULL for every table.  Returns the number of entries dropped.  (The Python front end:
 * earl_benchmark_amd.physics.DeviceModel.__del__; nothing in the reference corresponds -- MuJoCo reads `opt.cone` from the one model it holds.) */
int earl_physics_forget_table(const void* col);
int earl_debug_set_physics_lanes(int lanes_per_env);

/* ---------------------------------------------------------------------------------------------------------------------
 * Kitchen env step (BASELINE configs[3]).  Replaces, per env instance, PersistentStateWrapper.step
 * (wrappers/persistent_state_wrapper.py:17-31) o Kitchen.step (envs/kitchen.py:185-187) o KitchenV0.step
 * (envs/kitchen_assets/adept_envs/adept_envs/franka/kitchen_multitask_v0.py:91-125): action clip / scale and mocap update (:92-102), Robot.step
 * (franka/robot/franka_robot.py:178-207: velocity-limited position targets, do_simulation = frame_skip x mj_step with ctrl = the first nu = 2
 * targets), _get_obs with sensor noise (:127-139, franka_robot.py:137-168), Kitchen._get_reward_n_score / is_successful (kitchen.py:141-183).
 * The launches go to `stream` in order: promote + save, earl_kitchen_action, the nv = 23 stepper, failure guard, noise, earl_kitchen_obs,
 * earl_kitchen_reward, bookkeeping.  Everything is caller-owned device memory, scratch included. */
struct earl_kitchen_params;      /* include/earl_glue.h */
typedef struct earl_kitchen_cfg {
  int32_t n, env_offset;
  int32_t horizon;               /* <= 0: never done */
  int32_t frame_skip;            /* 40 (kitchen_multitask_v0.py:40) */
  int32_t sensor_noise;          /* 0: observations without noise (the reference's `initializing` mode) */
  int32_t n_att;                 /* attachments of the model (rows of st.att_xpos per env) */
  int32_t site_att[8];           /* attachment indices of knob1..4_site, light_site, slide_site, hinge_site2, microhandle_site (kitchen.py:148-155) */
  uint64_t seed, counter;        /* noise draws: Philox(seed; 0x4B00 + j / 2, global env id, counter) */
  const double* mocap_quat_dev;  /* device, [4]: the mocap body's (constant) orientation, used as given */
} earl_kitchen_cfg;
typedef struct earl_kitchen_state {
  double* qpos; double* qvel;    /* [n, 23] */
  double* mocap_pos;             /* [n, 3] */
  double* goal;                  /* [n, 23] the goal in force; read by every entry point, written by earl_kitchen_agents_rollout only (a handover of the agent pair) */
  double* last_qp_robot;         /* [n, 9] robot joints of the newest (noisy) observation: Robot_VelAct.ctrl_velocity_limits starts from them */
  double* att_xpos;              /* [n, n_att, 3] attachment positions the stepper leaves (kinematics of the last timestep's start) */
  int32_t* steps_since_reset;    /* [n] */
  int32_t* fail_count;           /* [n] may be NULL */
  double* last_obs;              /* [n, 46] */
  /* scratch, caller-owned like everything else: */
  double* action64;              /* [n, 9] */
  double* ctrl9;                 /* [n, 9] */
  double* noise;                 /* [n, 46] (may be NULL when sensor_noise == 0; otherwise earl_kitchen_step returns EARL_ERR_ARG) */
  double* qpos_bak; double* qvel_bak;   /* [n, 23] the state a diverged step is rolled back to */
  double* sites;                 /* [n, 8, 3] */
  uint8_t* bad;                  /* [n] */
  double* mocap_bak;             /* [n, 3] the mocap target before this step's action: a diverged step restores it (like earl_sawyer_out.status) */
  double* att_bak;               /* [n, n_att, 3] attachment positions before this step: a diverged step leaves att_xpos at them */
} earl_kitchen_state;
typedef struct earl_kitchen_out {
  double* obs;                   /* [n, 46] */
  double* reward;                /* [n] float64, like the reference's */
  uint8_t* done; uint8_t* success;
  uint8_t* status;               /* [n] may be NULL: EARL_STEP_DIVERGED as in earl_sawyer_out: state, mocap target and attachment positions are
                                    rolled back to the env's last stable ones, the row carries the last stable observation, reward 0 */
} earl_kitchen_out;
int earl_kitchen_step(const void* model24, const earl_collision_model* col, const struct earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                      const earl_kitchen_state* st, const float* action /* [n, 9] */, const earl_kitchen_out* out, earl_stream_t stream);

/* T env steps of every env in ONE launch: action [T, n, 9] float32, the rows of `out` are [T, n, ...].  Equal, bit for bit, to T calls of
 * earl_kitchen_step with cfg.counter, cfg.counter + 1, ... (state, scratch-free: action64 / ctrl9 / noise / qpos_bak / qvel_bak / sites / bad / mocap_bak /
 * att_bak of `st` are not used and may be NULL); every wave walks its envs through the whole rollout on its own, so the launch costs the slowest wave's SUM
 * over the T steps instead of T times the slowest wave of a step.  The lifelong wrapper's goal switch is not part of it (callers step those). */
int earl_kitchen_rollout(const void* model24, const earl_collision_model* col, const struct earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                         const earl_kitchen_state* st, const float* action /* [T, n, 9] */, int32_t T, const earl_kitchen_out* out, earl_stream_t stream);
/* As earl_kitchen_rollout, with the sensor-noise counter cfg->counter + clock[0], where `clock` is DEVICE memory holding two uint64 read when the kernel runs
 * (NULL = zero; clock[1] has no use here).  For graph capture, as earl_sawyer_rollout_clocked.  earl_kitchen_rollout is this with clock = NULL; the eight-launch
 * earl_kitchen_step has no clocked form (its noise comes from earl_philox_uniform with the host's counter). */
int earl_kitchen_rollout_clocked(const void* model24, const earl_collision_model* col, const struct earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                 const earl_kitchen_state* st, const float* action /* [T, n, 9] */, int32_t T, const uint64_t* clock, const earl_kitchen_out* out,
                                 earl_stream_t stream);
/* ---- closed loop: an MLP policy evaluated INSIDE the kitchen rollout kernel ----
 * T closed-loop env steps of every env in ONE launch of the kitchen rollout kernel: between two env steps the 32 lanes that own an env evaluate the policy, observation ->
 * float32 MLP 46 -> hidden (-> hidden) -> 9 -> action -> next env step, so the waves drift apart over the whole rollout as they do in earl_kitchen_rollout (a captured
 * loop of T one-step launches waits for the slowest wave T times).  earl_mlp_policy / earl_gaussian_head are earl_tabletop.h's, with dims[0] = 46 and dims[n_layers] = 9
 * (head = NULL) or 18 (head given: output rows 0..8 the mean, rows 9..17 the raw log_std); hidden widths multiples of 16 in 16..256; policy->params 16-byte aligned
 * (the rows of every layer after the first are read in 16-byte pieces; the input layer's rows, 184 bytes, are read element by element).
 * Per env and env step t, in this order:
 *   1. input: at t = 0 the env's row of obs0 [n, 46] (device); at t > 0 the row the env emitted at step t - 1 exactly as it stands in out->obs -- the sensor noise and
 *      the repeated row of a rolled-back step included (the same bits stand in the env's row of st->last_obs) -- each double rounded once to float32;
 *   2. network: the contract of earl_tabletop_policy_rollout (acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc); relu_f32, tanh_f32; the head's exp_f32,
 *      normal_quantile_f32, log_std maps and u = fmaf(exp_f32(ls), eps, mean): csrc/policy_math.h); earl_mlp_policy_forward_cpu above states it on the host;
 *   3. head: THREE Philox4x32-10 blocks per (env, env step), key = cfg->seed, block b in {0, 1, 2} with counter words {0x504F4C00 + b, cfg->env_offset + env, ev lo, ev hi},
 *      ev = cfg->counter + clock[0] + t (the step's sensor-noise counter; the noise's draw indices are 0x4B00 + j: the streams are disjoint); words x, y, z, w of block b ->
 *      action dimensions 4 b .. 4 b + 3 (block 2: x only), each as normal_quantile_f32(word >> 8);
 *   4. stores: actions[t] ([T, n, 9] device, required) and head->eps_out[t] ([T, n, 9] or NULL, written in both modes);
 *   5. the env step of earl_kitchen_rollout_clocked on exactly the float32 values stored in actions[t], through its own clip to [-1, 1] -- the reference clips silently
 *      (kitchen_multitask_v0.py:92), so an unbounded policy (out_act == EARL_ACT_NONE) is taken, unlike on the minitaur -- then failure guard, rollback of the state and
 *      the mocap target, noise, reward, bookkeeping: the same statements.
 * The launch is therefore bit-identical to earl_kitchen_rollout_clocked fed with the actions it returns: every array of `out`, qpos, qvel, mocap_pos, last_qp_robot,
 * last_obs, att_xpos, steps_since_reset, fail_count.  clock as for earl_kitchen_rollout_clocked (may be NULL).  The launch form is picked by that entry point's rule
 * (earl_debug_set_solo: two envs per wave, one env per wave, one env per workgroup on one, four or two waves; in the several-wave forms the env's owner wave evaluates the
 * policy); all five forms return the same bits.
 * EARL_ERR_ARG before any HIP call: everything earl_kitchen_rollout_clocked refuses, the policy and head rules of earl_tabletop.h's argument contract with the widths
 * 46 / 9, and this entry point's own: NULL policy / obs0 / actions, policy->params not 16-byte aligned.  n = 0 or T = 0: EARL_OK, nothing launched.
 * The lifelong wrapper's goal switch is not part of it, as for earl_kitchen_rollout.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned; each widens exactly (u << 16) into the same fmaf chain, so the
 * launch returns the bits of the fp32 launch fed with the widened values. */
int earl_kitchen_policy_rollout(const void* model24, const earl_collision_model* col, const struct earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_gaussian_head* head, const double* obs0, int32_t T,
                                const uint64_t* clock, float* actions, const earl_kitchen_out* out, earl_stream_t stream);
/* ---- the same closed loop for a POPULATION of policies, with per-env episode summaries and without any [T] array ----
 * earl_policy_population / earl_episode_summary are earl_tabletop.h's, as they are.  One episode per launch: the summary rows are [n].
 *   pop      NULL = one policy: bit-identical to earl_kitchen_policy_rollout, which is this call with pop = summary = NULL.  Otherwise the env with GLOBAL id
 *            g = cfg->env_offset + i runs member g / G, whose parameters start at policy->params + (g / G) * param_stride.  The member depends on the global id only: not on
 *            n, the shard split, the launch form, or which wave or 32-lane group holds the env; env_offset need not be a multiple of anything, and a wave whose two envs
 *            belong to two members is correct, only slower.  The launch is bit-identical to cutting the batch at the global ids that are multiples of G and running
 *            earl_kitchen_policy_rollout on each piece (env_offset = its first global id, n = its length, the matching state rows) with that member's parameters:
 *            outputs, actions, eps_out, every state row, fail_count, counters.
 *   summary  NULL, or rows [n]: ret = sum over t ascending of reward_t (float64, the doubles as out->reward holds or would hold them); success_last = the success flag of
 *            step T - 1; first_success = the smallest t with success, or -1.  Rolled-back rows count with reward 0 and success 0.  The lane that stores the env's reward
 *            keeps the three words up to date in device memory after every env step (step 0 initialises them); nothing of them lives in a register across a timestep.
 *   actions and every pointer of `out`, out->obs included, may be NULL (`out` itself may not).  With out->obs == NULL the env's row of st->last_obs -- which every
 *            kitchen rollout keeps current step by step, and a rolled-back step leaves standing -- is the row the policy of step t + 1 reads, each lane reading what it
 *            stored itself, behind the fence that ends an env step.  The state left behind, last_obs included, equals the full launch's.
 * In the several-wave forms the env's owner wave does the policy phase and the summary stores; a 32-lane group that is not live (an idle group of the last wave, a
 * one-env-per-wave launch's shadow) evaluates on zeros with the rows of the member of the env it shadows, which is always an env of the batch.
 * EARL_ERR_ARG before any HIP call: everything earl_kitchen_policy_rollout refuses (but NULL actions / out pointers), the contract's population rules with group size 16
 * (csrc/policy_check.h: check_population, the member range against the global ids included), param_stride % 4 != 0 (every member's rows are read in 16-byte pieces).
 * st->last_obs is required as ever.  n = 0 or T = 0: EARL_OK, nothing launched.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_kitchen_population_rollout(const void* model24, const earl_collision_model* col, const struct earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                    const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_gaussian_head* head,
                                    const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_kitchen_out* out,
                                    const earl_episode_summary* summary, earl_stream_t stream);
/* ---- the forward / reset AGENT PAIR inside the same launch: a POPULATION of pairs, a TABLE of backward goals, episode SUMMARIES -- each NULL or given ----
 * earl_agent_pair is earl_tabletop.h's struct and earl_backward_goals the one above, as they are, with the kitchen's sizes: a goal row is 23 doubles (a qpos: a row of
 * st->goal), pair->backward_goal ONE such row, goals->table [n_rows, 23], forward_goals [n_forward_goals, 23] (device); agent_out [T, n]; forward_success /
 * backward_success [n] (one launch is one episode).  policy->params is [2, pair->param_stride] -- row 0 the forward agent, row 1 the reset agent, both of policy's
 * architecture and head -- or, with pop, [P, 2, pair->param_stride] at pop->param_stride.  pair = NULL is refused: it is not an alias of earl_kitchen_population_rollout.
 * Per env and env step t, in this order (the order is the contract; the six items are earl_sawyer_pair_rollout's):
 *   1. the action is computed from the observation the env last emitted (earl_kitchen_policy_rollout's rule: obs0 at step 0, afterwards the row of step t - 1 as it
 *      stands, the goal block a handover patched included) by the network of the env's current `phase` (0 forward, anything else reset) of its member, at
 *      policy->params + (g / G) * pop->param_stride + phase * pair->param_stride; the arithmetic is unchanged;
 *   2. with a head, the step's THREE Philox blocks are the ones earl_kitchen_policy_rollout makes ({0x504F4C00 + b, global id, ev}, ev = cfg->counter + clock[0] + t):
 *      they do not depend on the phase;
 *   3. agent_out[t n + env], actions and eps_out are written;
 *   4. the env step runs as in the single-policy kernel, failure guard, rollback and fail_count included; reward and success refer to the goal in force DURING the
 *      step: the reward reads the goal from the observation as emitted, before any patch;
 *   5. steps_in_phase += 1 (a rolled-back step counts, with success 0), and the env hands over if (switch_on_success && success) || steps_in_phase >=
 *      switch_every[phase]: phase ^= 1, steps_in_phase = 0; forward_success / backward_success of the phase that ended is incremented if switch_on_success && success
 *      (a step where the clock ran out as well counts as ended by success); step 0 of the launch starts both counters at 0.
 *      Entering the reset phase, the env's row of st->goal becomes pair->backward_goal, or with `goals` table[r], r = min((int)(u01(b.x, b.y) * n_rows), n_rows - 1), where
 *      b is the Philox4x32-10 block {0xFFFD, global env id, ev lo, ev hi} under key cfg->seed (earl_sawyer_agents_rollout's draw, with this env's ev; the sensor noise
 *      draws with 0x4B00 + j, the head with 0x504F4C00 + b); goals->row[env] = r and row_out[t n + env] = r at such a step, row_out is -1 at every other step of a live
 *      env; with neither the goal stays.  Entering the forward phase with forward_goals, it becomes forward_goals[r], r from the 0xFFFE draw of the same form over
 *      n_forward_goals rows (one row: r = 0 whatever the draw, so a table of one row is a fixed row); without, the goal stays.  Whenever the row changes, entries
 *      23 .. 45 of this step's emitted observation row are patched, in row t of out->obs if given AND in the env's row of st->last_obs, which the kitchen always keeps:
 *      the next action sees the new goal, this step's reward used the old one;
 *   6. phase and steps_in_phase are stored after every env step; in the several-wave forms the env's owner wave does all of this.  st->goal is left as the goal in
 *      force at launch exit: there is no separate entry rule, and every other entry point keeps working on the state.
 * Identities: never switching (switch_every > T, switch_on_success = 0) with all envs in phase 0 is bit-identical to earl_kitchen_population_rollout with row 0 of every
 * member -- outputs, actions, eps, state, fail_count, summary; all envs in phase 1 with no backward goal, to the same with row 1.  pop equals cutting the batch at the
 * global ids that are multiples of G.  summary equals its definitions.  A `goals` table of ONE row equals pair->backward_goal = that row.  Nothing depends on n, the
 * shard split, the launch form (all five of earl_debug_set_solo) or how T steps are cut into launches.  actions, every pointer of `out`, the pair's three output pointers
 * and goals->row / row_out may be NULL.
 * EARL_ERR_ARG before any HIP call: everything earl_kitchen_population_rollout refuses, the contract's pair rules (csrc/policy_check.h: NULL pair / phase /
 * steps_in_phase, switch_every < 1, switch_on_success other than 0 / 1, param_stride below the parameter count), param_stride % 4 != 0, pop->param_stride <
 * 2 * pair->param_stride, goals with a NULL table or n_rows < 1, goals together with pair->backward_goal, n_forward_goals < 0, and a backward goal or table given with
 * forward_goals == NULL or n_forward_goals < 1 (the forward goal could not be restored).  n = 0 or T = 0: EARL_OK, nothing launched.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_kitchen_agents_rollout(const void* model24, const earl_collision_model* col, const struct earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_policy_population* pop,
                                const earl_backward_goals* goals, const double* forward_goals, int32_t n_forward_goals, const earl_gaussian_head* head, const double* obs0,
                                int32_t T, const uint64_t* clock, float* actions, const earl_kitchen_out* out, const earl_episode_summary* summary, earl_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Minitaur env (BASELINE configs[4]) on the same stepper: floating base + 16 hinges (nv = 22, nq = 23), four connect
 * constraints (the knee closures), spheres against the ground and the wall tiles; the rigid-body MODEL is this build's own authoring
 * (tools/minitaur_model.py: the reference's URDF is not in its tree) -- parity with the reference's PyBullet simulation is UNPINNED AND MODEL-LESS.
 * Replaces, per env instance, PersistentStateWrapper.step (wrappers/persistent_state_wrapper.py:17-31) o GoalConditionedMinitaurBulletEnv.step
 * (envs/minitaur_gym_env.py:505-546 over MinitaurBulletEnv.step :285-329): Minitaur.ConvertFromLegModel (envs/minitaur.py:434-457), then
 * num_substeps x { Minitaur.ApplyAction (:326-390: velocity-limit clip of the command, MotorModel.convert_to_torque envs/motor.py:49-94, overheat
 * protection, torque x motor direction); one timestep of the stepper }, _reward, is_successful, GetObservation (:300-324) + goal; and
 * reset (:222-270, :476-479): goal drawn from goal_table, [UPSTREAM MinitaurEnvRandomizer, ranges from memory] per cfg.randomize: battery voltage, motor viscous
 * damping, base / leg-link / motor masses, foot friction (the setters are the reference's own, envs/minitaur.py:468-508), pose <- reset_qpos, settle_steps x (ApplyAction(pi / 2), timestep).
 * obs [32] float64: motor angles 8, motor velocities 8, observed motor torques 8 (all in motor space = joint x direction), base orientation (x, y, z, w),
 * base x y, goal x y. */
typedef struct earl_minitaur_cfg {
  int32_t n, env_offset;
  int32_t horizon;                 /* <= 0: never done */
  int32_t num_substeps;            /* 5  (minitaur_gym_env.py:25, 161-164) */
  int32_t settle_steps;            /* 100 (:265-269) */
  int32_t randomize;               /* MinitaurEnvRandomizer [UPSTREAM pybullet_envs.bullet.minitaur_env_randomizer] per reset, bit mask: 1 battery voltage U(14.8, 16.8) and
                                      motor viscous damping U(0, 0.01) (else 16 V, 0); 2 base / leg-link / motor masses (minitaur.py:468-488); 4 foot friction (:490-498) */
  int32_t n_goals;                 /* rows of goal_table: 12 (:467-469) */
  int32_t goal_change_frequency;   /* > 0: LifelongWrapper.step (lifelong_wrapper.py:30-44), as in earl_sawyer_cfg */
  int32_t overheat_steps;          /* OVERHEAT_SHUTDOWN_TIME / time_step = 500 (minitaur.py:14-15, 356) */
  int32_t motor_dof[8];            /* dof of motor i (MOTOR_NAMES order, minitaur.py:18-22) */
  int32_t pad_;
  double motor_dir[8];             /* minitaur.py:80 */
  double motor_kp, motor_kd;       /* 1.0, 0.02 (minitaur_gym_env.py:85-86) */
  double motor_velocity_limit;     /* 150 (:472) */
  double overheat_torque;          /* 2.45 */
  double distance_weight, energy_weight;   /* 2.0, 0.005 (:473, :71) */
  double success_radius;           /* 0.1 (:500) */
  const double* goal_table;        /* device, [n_goals, 2] */
  const double* reset_qpos;        /* device, [23]: base (0, 0, 0.2), identity, motor joints dir pi / 2, knee joints dir -2.1834 (minitaur.py:10-11, 187-211) */
  double base_mass_err[2];         /* (-0.2, 0.2): SetBaseMass(U(m (1 + lo), m (1 + hi))) -> the root body's mass and inertia x that factor */
  double leg_mass_err[2];          /* (-0.2, 0.2): SetLegMasses([U of the leg-link mass, U of the motor mass]): minitaur.py:472-488 writes the FIRST to all 16 leg links --
                                      upper AND lower -- and the second to the 8 motors.  This build's links: upper = motor + upper leg link -> mass (and inertia) x
                                      (motor' + leg') / model mass; lower -> x leg' / model mass (the reference's quirk kept: a lower leg then weighs what an upper one does) */
  double leg_mass, motor_mass;     /* the two masses the randomizer reads back from the URDF (minitaur.py:101-107): leg link LEG_LINK_ID[0], motor MOTOR_LINK_ID[0] */
  double foot_friction[2];         /* (0.8, 1.5): SetFootFriction -> friction of every contact of a lower-leg link's spheres (FOOT_LINK_ID = the lower links) */
  uint64_t seed, counter;          /* reset draws: Philox(seed; 0x4D00 + k, global env id, counter), k = 0 goal, 1 voltage, 2 damping, 3 base mass, 4 leg-link mass,
                                      5 motor mass, 6 foot friction */
  uint64_t step_counter;           /* env steps taken before this launch (goal-switch draws: Philox(seed; 0xFFFE, global env id, step)) */
} earl_minitaur_cfg;
typedef struct earl_minitaur_state {
  double* qpos;                    /* [n, 23] */
  double* qvel;                    /* [n, 22] */
  double* goal;                    /* [n, 2] */
  double* motor_param;             /* [n, 6] what the randomizer set at the last reset: battery voltage, motor viscous damping, mass factor of the base, of the upper
                                      links, of the lower links, foot friction (<= 0: the contact classes' own) */
  double* observed_torque;         /* [n, 8] Minitaur._observed_motor_torques of the newest ApplyAction */
  int32_t* overheat;               /* [n, 8] Minitaur._overheat_counter */
  uint8_t* motor_enabled;          /* [n, 8] Minitaur._motor_enabled_list */
  int32_t* steps_since_reset;      /* [n] */
  int32_t* steps_since_goal_change;   /* [n]; may be NULL when cfg.goal_change_frequency == 0 (otherwise the rollout and the reset return EARL_ERR_ARG) */
  int32_t* fail_count;             /* [n] may be NULL */
  double* last_obs;                /* [n, 32] may be NULL (as in earl_sawyer_state: NaN rows when the first step of a launch diverges) */
} earl_minitaur_state;
typedef struct earl_minitaur_out {
  double* obs;                     /* [T, n, 32] */
  double* reward;                  /* [T, n] float64, like the reference's */
  uint8_t* done; uint8_t* success;
  uint8_t* status;                 /* [T, n] may be NULL: EARL_STEP_DIVERGED as in earl_sawyer_out (state rolled back, last stable observation, reward 0) */
} earl_minitaur_out;
/* T env steps of every env in ONE launch; action float32 [T, n, 8] in [-1, 1] (the reference raises ValueError beyond +-1.01: the Python front end
 * checks; the kernel clips to +-1.01).  Solver start: as earl_physics_step states it, every env step starting cold; within an env step a contact slot that holds the
 * same collision pair as at the timestep before starts from the edge set its passes ENDED with (same fixed point, fewer passes: 2.05 -> 1.66 per timestep on random actions). */
int earl_minitaur_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                          const float* action, int32_t T, const earl_minitaur_out* out, earl_stream_t stream);
/* As earl_minitaur_rollout, with the goal-switch counter cfg->step_counter + clock[1], where `clock` is DEVICE memory holding two uint64 read when the kernel
 * runs (NULL = zero; the rollout draws with step_counter only: clock[0] has no use here).  For graph capture, as earl_sawyer_rollout_clocked.  Every rollout
 * kernel honours it: the two-wave and one-wave kernels and the generic stepper (earl_debug_set_minitaur_stepper(0)).  earl_minitaur_rollout is this with clock = NULL. */
int earl_minitaur_rollout_clocked(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                  const float* action, int32_t T, const uint64_t* clock, const earl_minitaur_out* out, earl_stream_t stream);
/* ---- closed loop: an MLP policy evaluated INSIDE the minitaur rollout kernels ----
 * T closed-loop env steps in ONE launch: between two env steps the 32 lanes that own an env evaluate the policy, observation -> float32 MLP 32 -> hidden (-> hidden) -> 8
 * -> action -> next env step.  earl_mlp_policy / earl_gaussian_head are earl_tabletop.h's, with dims[0] = 32 and dims[n_layers] = 8 (head = NULL) or 16 (head given:
 * output rows 0..7 the mean, rows 8..15 the raw log_std); hidden widths multiples of 16 in 16..256; policy->params 16-byte aligned (weight rows are read in 16-byte pieces).
 * Per env and env step t, in this order:
 *   1. input: at t = 0 the env's row of obs0 [n, 32] (device); at t > 0 row t - 1 of THIS launch's out->obs exactly as emitted -- the repeated row of a rolled-back step
 *      and the goal entries 30 / 31 patched by a lifelong goal switch included -- each double rounded once to float32;
 *   2. network: the contract of earl_tabletop_policy_rollout (acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc); relu_f32, tanh_f32; the head's exp_f32,
 *      normal_quantile_f32, log_std maps and u = fmaf(exp_f32(ls), eps, mean): csrc/policy_math.h); earl_mlp_policy_forward_cpu below states it on the host;
 *   3. head: TWO Philox4x32-10 blocks per (env, env step), key = cfg->seed, block b in {0, 1} with counter words {0x504F4C00 + b, cfg->env_offset + env, ev lo, ev hi},
 *      ev = cfg->step_counter + clock[1] + t (the value the goal-switch draw of that step uses; its draw index is 0xFFFE, the reset's are 0x4D00 .. 0x4D06: the streams
 *      are disjoint); words x, y, z, w of block b -> action dimensions 4 b .. 4 b + 3, each as normal_quantile_f32(word >> 8);
 *   4. stores: actions[t] ([T, n, 8] device, required) and head->eps_out[t] ([T, n, 8] or NULL, written in both modes);
 *   5. the env step of earl_minitaur_rollout_clocked on exactly the float32 values stored in actions[t] (clipped to +-1.01, leg model, failure guard, rollback, reward,
 *      success, done, goal switch, state rows: the same statements).
 * The launch is therefore bit-identical to earl_minitaur_rollout_clocked fed with the actions it returns: outputs, state rows, fail_count, last_obs, counters.
 * clock as for earl_minitaur_rollout_clocked (may be NULL).  The kernel is picked by the plain entry point's rule (one-wave kernel in its three launch shapes, two-wave
 * kernel; earl_debug_set_solo_mt, earl_debug_set_minitaur_duo); both forms return the same bits.
 * EARL_ERR_ARG before any HIP call: everything earl_minitaur_rollout_clocked refuses, the policy and head rules of earl_tabletop.h's argument contract with the widths
 * 32 / 8, and this entry point's own: NULL policy / obs0 / actions, policy->params not 16-byte aligned, and out_act != EARL_ACT_TANH: the reference env raises on an
 * action outside +-(1 + 0.01), a kernel cannot, and the open-loop replay of the returned actions must not raise either, so the minitaur takes bounded policies only.
 * The generic-stepper comparison build
 * (earl_debug_set_minitaur_stepper(0)) has no policy form: EARL_ERR_ARG.  n = 0 or T = 0: EARL_OK, nothing launched.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned; each widens exactly (u << 16) into the same fmaf chain, so the
 * launch returns the bits of the fp32 launch fed with the widened values. */
int earl_minitaur_policy_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                 const earl_mlp_policy* policy, const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions,
                                 const earl_minitaur_out* out, earl_stream_t stream);
/* ---- the same closed loop for a POPULATION of policies, with per-env episode summaries and without any [T] array ----
 * earl_policy_population / earl_episode_summary are earl_tabletop.h's, as they are.  One episode per launch: the summary rows are [n].
 *   pop      NULL = one policy: bit-identical to earl_minitaur_policy_rollout, which is this call with pop = summary = NULL.  Otherwise the env with GLOBAL id
 *            g = cfg->env_offset + i runs member g / G, whose parameters start at policy->params + (g / G) * param_stride.  The member depends on the global id only: not on
 *            n, the shard split, the launch form (one-wave kernel in its three shapes, two-wave kernel), or which wave or 32-lane group holds the env; env_offset need not
 *            be a multiple of anything, and a wave whose two envs belong to two members is correct, only slower.  The launch is bit-identical to cutting the batch at the
 *            global ids that are multiples of G and running earl_minitaur_policy_rollout on each piece (env_offset = its first global id, n = its length, the matching
 *            state rows) with that member's parameters: outputs, actions, eps_out, every state row, fail_count, counters.
 *   summary  NULL, or rows [n]: ret = sum over t ascending of reward_t (float64, the doubles as out->reward holds or would hold them); success_last = the success flag of
 *            step T - 1; first_success = the smallest t with success, or -1.  Rolled-back rows count with reward 0 and success 0.  Lane 0 of the env, which stores its
 *            reward, keeps the three words up to date in device memory after every env step (step 0 initialises them); nothing of them lives in a register across a timestep.
 *   actions and every pointer of `out`, out->obs included, may be NULL (`out` itself may not).  With out->obs == NULL the env's row of st->last_obs (then required; with
 *            out->obs it may be NULL as ever) is the one observation row the launch keeps: every emitted row is written to it, a rolled-back step leaves it standing, a goal
 *            switch patches its entries 30 / 31, and the policy of step t + 1 reads it, each lane reading what it stored itself, behind the fence that ends an env step.
 *            The state left behind, last_obs included, equals the full launch's.
 * A 32-lane group that is not live (an idle group of the last wave or workgroup, a one-env-per-wave launch's shadow) evaluates on zeros with the rows of the member of the
 * env it shadows, which is always an env of the batch: no id at or beyond cfg->env_offset + n is ever formed.
 * EARL_ERR_ARG before any HIP call: everything earl_minitaur_policy_rollout refuses (but NULL actions / out pointers) -- bounded policies only and no generic-stepper form
 * included --, the contract's population rules with group size 16 (csrc/policy_check.h: check_population, the member range against the global ids included),
 * param_stride % 4 != 0 (every member's rows are read in 16-byte pieces), out->obs == NULL with st->last_obs == NULL.  n = 0 or T = 0: EARL_OK, nothing launched.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_minitaur_population_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                     const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_gaussian_head* head, const double* obs0, int32_t T,
                                     const uint64_t* clock, float* actions, const earl_minitaur_out* out, const earl_episode_summary* summary, earl_stream_t stream);
/* ---- the forward / reset AGENT PAIR inside the same launch: a POPULATION of pairs, a TABLE of backward goals, episode SUMMARIES -- each NULL or given ----
 * earl_agent_pair is earl_tabletop.h's struct and earl_backward_goals the one above, as they are, with the minitaur's sizes: a goal row is 2 doubles (x, y: a row of
 * st->goal), pair->backward_goal ONE such row, goals->table [n_rows, 2]; agent_out [T, n]; forward_success / backward_success [n] (one launch is one episode).
 * policy->params is [2, pair->param_stride] -- row 0 the forward agent, row 1 the reset agent, both of policy's architecture and head -- or, with pop,
 * [P, 2, pair->param_stride] at pop->param_stride.  pair = NULL is refused: it is not an alias of earl_minitaur_population_rollout.
 * Per env and env step t, in this order (the order is the contract; the six items are earl_sawyer_pair_rollout's):
 *   1. the action is computed from the observation the env last emitted (earl_minitaur_policy_rollout's rule: obs0 at step 0, afterwards row t - 1 as it stands, the goal
 *      entries a handover patched included) by the network of the env's current `phase` (0 forward, anything else reset) of its member, at
 *      policy->params + (g / G) * pop->param_stride + phase * pair->param_stride; the arithmetic is unchanged;
 *   2. with a head, the step's TWO Philox blocks are the ones earl_minitaur_policy_rollout makes ({0x504F4C00 + b, global id, ev}, ev = cfg->step_counter + clock[1] + t):
 *      they do not depend on the phase;
 *   3. agent_out[t n + env], actions and eps_out are written;
 *   4. the env step runs as in the single-policy kernels, failure guard, rollback and fail_count included; reward and success refer to the goal in force DURING the
 *      step, which is the env's row of st->goal;
 *   5. steps_in_phase += 1 (a rolled-back step counts, with success 0), and the env hands over if (switch_on_success && success) || steps_in_phase >=
 *      switch_every[phase]: phase ^= 1, steps_in_phase = 0; forward_success / backward_success of the phase that ended is incremented if switch_on_success && success
 *      (a step where the clock ran out as well counts as ended by success); step 0 of the launch starts both counters at 0.
 *      Entering the reset phase, the env's row of st->goal becomes pair->backward_goal, or with `goals` table[r], r = min((int)(u01(b.x, b.y) * n_rows), n_rows - 1), where
 *      b is the Philox4x32-10 block {0xFFFD, global env id, ev lo, ev hi} under key cfg->seed (earl_sawyer_agents_rollout's draw: the counter words, u01 and clamp of the
 *      0xFFFE draw; index 0xFFFD is free here too: the reset draws with 0x4D00 .. 0x4D06, the head with 0x504F4C00 / 0x504F4C01); goals->row[env] = r and
 *      row_out[t n + env] = r at such a step, row_out is -1 at every other step of a live env; with neither the goal stays.  Entering the forward phase, it becomes the
 *      cfg->goal_table row of the 0xFFFE draw of this step, the lifelong switch's expression.  Whenever the row changes, entries 30 / 31 of this step's emitted observation
 *      row (row t of out->obs, or the carried row of st->last_obs) are patched: the next action sees the new goal, this step's reward used the old one;
 *   6. phase and steps_in_phase are stored after every env step (in the two-wave kernel by the first-half wave, next to the goal switch; the new goal is the one its
 *      later steps observe).  st->goal is left as the goal in force at launch exit: there is no separate entry rule, and every other entry point keeps working on the state.
 * The pair's handover IS the goal switch of autonomous RL: cfg->goal_change_frequency > 0 is refused (the lifelong switch and a forward entry would both draw with index
 * 0xFFFE at the same step; running both is not offered).
 * Identities: never switching (switch_every > T, switch_on_success = 0) with all envs in phase 0 is bit-identical to earl_minitaur_population_rollout with row 0 of every
 * member -- outputs, actions, eps, state, fail_count, summary; all envs in phase 1 with no backward goal, to the same with row 1.  pop equals cutting the batch at the
 * global ids that are multiples of G.  summary equals its definitions, reward and success against the goal in force during the step.  A `goals` table of ONE row equals
 * pair->backward_goal = that row.  Nothing depends on n, the shard split, the launch form (one-wave kernel in its three shapes, two-wave kernel) or how T steps are cut into
 * launches.  actions, every pointer of `out`, the pair's three output pointers and goals->row / row_out may be NULL.
 * EARL_ERR_ARG before any HIP call: everything earl_minitaur_population_rollout refuses (no generic-stepper form included), the contract's pair rules
 * (csrc/policy_check.h: NULL pair / phase / steps_in_phase, switch_every < 1, switch_on_success other than 0 / 1, param_stride below the parameter count), param_stride
 * % 4 != 0, pop->param_stride < 2 * pair->param_stride, goals with a NULL table or n_rows < 1, goals together with pair->backward_goal, cfg->goal_change_frequency > 0.
 * n = 0 or T = 0: EARL_OK, nothing launched.
 * policy->precision == EARL_PRECISION_BF16 (earl_tabletop.h): params holds uint16_t bf16 values, 16-byte aligned, every param_stride counts those elements and is a multiple
 * of 8; each value widens exactly (u << 16) into the same fmaf chain, so the launch returns the bits of the fp32 launch fed with the widened values. */
int earl_minitaur_agents_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                 const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_policy_population* pop, const earl_backward_goals* goals,
                                 const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_minitaur_out* out,
                                 const earl_episode_summary* summary, earl_stream_t stream);

/* ---- branches on the minitaur: K candidate action sequences per env scored from the CURRENT state in one launch, the state left as it is ----
 * earl_sawyer_branch_rollout's contract restated for this env: K plans of H steps per env, one return, one success flag, one first-success step, one last observation
 * and one count of rolled-back steps each, nothing kept.  ONE launch of the rollout kernel over the K n virtual envs v = k n + i (branch k of env i), in front of it
 * one small kernel that copies the env's [n] state rows into the workspace's [K n]; no [H] row is written anywhere.
 *   equivalence  branch (k, i) equals earl_minitaur_rollout_clocked(model24, col, cfg, <a private copy of st>, act + k * act_branch_stride, H, clock, out) restricted to
 *                env i, bit for bit:  summary->ret[k n + i] = the float64 sum over t ascending of out->reward[t][i] (a rolled-back step adds 0);  success_last =
 *                out->success[H - 1][i];  first_success = the first t with success, or -1;  last_obs[k][i] = out->obs[H - 1][i] exactly as emitted -- entries 30 / 31
 *                as a lifelong switch patched them, the repeated row of a rolled-back step and, when step 0 itself diverges, the env's row of st->last_obs (NaN if
 *                that is NULL) included;  fail[k n + i] = the number of steps with status == EARL_STEP_DIVERGED.  A rolled-back step restores the BRANCH's own last
 *                stable state (qpos, qvel, the motors' overheat counters, enabled flags and observed torques); before its first stable step that is the state in `st`.
 *   draws        step t of EVERY branch uses the counter cfg->step_counter + clock[1] + t, and the Philox id is the env's global id cfg->env_offset + i, never the
 *                virtual index: all branches of an env see the lifelong goal draws (stream 0xFFFE) the env's next rollout will see.
 *   act          float32, device, [K, H, n, 8] in [-1, 1] (the kernel clips to +-1.01 as the rollout does).  act_branch_stride (in floats) == H * n * 8: a contiguous
 *                array; 0: every branch replays one [H, n, 8] block.
 *   state        `st` is read and never written: qpos, qvel, goal, motor_param, observed_torque, overheat, motor_enabled, the goal-switch counter, last_obs; no counter
 *                moves (steps_since_reset and fail_count are not even read).
 *   ws           what the launch mutates, per virtual env: the last stable qpos [23] and qvel [22], the goal, the eight motors' overheat counters, motor_enabled and
 *                observed_torque, the goal-switch counter and the one carried observation row (last_obs itself when given); motor_param, which a branch only reads,
 *                is copied beside them.  ONE device block: base 8-byte aligned, bytes >= what earl_minitaur_branch_ws_bytes(K, n, &bytes) reports (0 for K n == 0;
 *                monotone in K and in n); the call carves it and refuses a block that is too small.  The caller prepares NOTHING in it and nothing in it outlives the
 *                call.  No allocation, no host synchronisation: after one eager call with the same `col` (the friction-cone check reads the table's cone word once per
 *                address) the call can be captured into a HIP graph.
 *   outputs      summary (rows [K n]; the struct or any of its three pointers NULL), last_obs ([K, n, 32] or NULL) and fail ([K n] or NULL) in any combination, but not
 *                all five pointers NULL.
 *   forms        chosen by the number of VIRTUAL envs K n with earl_minitaur_rollout's rules: the tree-structured one-wave kernel in its three launch shapes and the
 *                two-waves-per-SIMD kernel (earl_debug_set_solo_mt and earl_debug_set_minitaur_duo force them as they force the rollout's).  Those forms are held
 *                bit-identical to each other, which is what makes the equivalence above independent of K.  Under earl_debug_set_minitaur_stepper(0) the call returns
 *                EARL_ERR_ARG: the generic build agrees with the tree-structured one to rounding only, like the policy form.
 * EARL_ERR_ARG before any HIP call, with a message in earl_last_error, for: everything earl_minitaur_rollout_clocked refuses in model / cfg / st; act or ws NULL; K < 0;
 * H < 0; a negative stride, or one that is neither 0 nor >= H * n * 8; all five outputs NULL; K * n beyond 2^31 - 1; with K n > 0: ws->base NULL or misaligned, ws->bytes
 * too small.  n == 0, K == 0 or H == 0 returns EARL_OK, launches nothing and writes nothing. */
typedef struct earl_minitaur_branch_ws {
  void*   base;    /* device, 8-byte aligned; NULL-able if K n == 0 */
  int64_t bytes;   /* size of the block at `base` */
} earl_minitaur_branch_ws;
/* *bytes = the size of the workspace of a branch launch of K branches of n envs; EARL_ERR_ARG for bytes == NULL, K < 0, n < 0, K * n beyond 2^31 - 1 */
int earl_minitaur_branch_ws_bytes(int32_t K, int32_t n, int64_t* bytes);
int earl_minitaur_branch_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                 int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_minitaur_branch_ws* ws,
                                 const earl_episode_summary* summary, double* last_obs, int32_t* fail, earl_stream_t stream);

/* ---- MPPI planning on the minitaur: I iterations of sample -> score -> reweight on the device, the env left as it is ----
 * earl_sawyer_plan_mppi's contract with EIGHT action dimensions, around earl_minitaur_branch_rollout, untouched.  Per iteration on the caller's stream: the candidates
 * kernel, earl_minitaur_branch_rollout (its replicate kernel and its rollout kernel), the update kernel; no allocation, no host synchronisation: after one eager call
 * with the same `col` (the branch launch's rule) the call can be captured into a HIP graph.  noise_counter is a host word: a captured call replays the same noise.
 * For iteration j = iteration0 + i (i = 0 .. iterations - 1), env `env` with global id g = cfg->env_offset + env, and the plan entering the iteration `mean` (the
 * argument for i = 0, the previous iteration's result afterwards):
 *   1 clipped mean  m[t][d] = clip(mean[t][d]) in float32 for d = 0 .. 7, clip(x) = (y = x > -1 ? x : -1; y < 1 ? y : 1) = min(max(x, -1), 1): every candidate lies
 *                   inside the env's +-1 action bound.
 *   2 candidates    branch 0 is the plan itself, a_0 = m.  For k >= 1: a_k[t][d] = clip(fmaf(sigma[d], eps_d, m[t][d])), eps_d = normal_quantile_f32(word_d >> 8)
 *                   (csrc/policy_math.h; earl_normal_quantile_f32).  TWO Philox4x32-10 blocks, key = cfg->seed: words x, y, z, w of the block with counter words
 *                   {0x504C4E00 | j, g, (k << 16) | t, noise_counter} serve d = 0 .. 3 -- the Sawyer planner's block: with equal seed, g, j, k, t, noise_counter, sigma
 *                   and mean, words 0 .. 3 of a minitaur candidate are the Sawyer candidate's --, those of the block with bit 31 of word 2 set,
 *                   {0x504C4E00 | j, g, 0x80000000 | (k << 16) | t, noise_counter}, serve d = 4 .. 7.  The bit is free: k <= 8191 < 2^15, t < 2^16.  Word 0 collides with
 *                   no other draw of the minitaur (the reset's 0x4D00 .. 0x4D06, the goal switch's 0xFFFE, the pair's 0xFFFD, the Gaussian head 0x504F4C00).  The draws
 *                   depend on (seed, g, j, k, t, noise_counter) only: not on n, not on the shard split.  The candidates live in memory, [K, H, n, 8] float32.
 *   3 scores        ret[k][env] = summary->ret of earl_minitaur_branch_rollout fed with those candidates (act_branch_stride = H * n * 8) and the caller's `clock`: goal
 *                   switches inside the look-ahead and rolled-back steps (reward 0) count exactly as that call defines them.  The minitaur's reward is dense and
 *                   NEGATIVE (distance and energy terms): a rolled-back step scores 0, above an honest one -- `fail` tells which branches had any.
 *   4 weights       beta = max_k ret[k];  x_k = (float)((ret[k] - beta) * inv_temperature) (two float64 roundings);  w_k = exp_f32(x_k) (csrc/policy_math.h;
 *                   earl_exp_f32);  W_k = (double)w_k * 2^24 rounded to nearest-even as int64 (0 .. 2^24);  S = sum_k W_k (>= 2^24: the best branch has W = 2^24).
 *   5 update        delta = a_k[t][d] - m[t][d] (one float32 subtraction);  D_k = (double)delta * 2^20 rounded to nearest-even as int64;  A = sum_k W_k * D_k in
 *                   int64 per dimension (|A| < 2^59 for K <= 8192);  mean'[t][d] = clip(m[t][d] + (float)((double)A / ((double)S * 2^20))), (double)A rounded to
 *                   nearest.  Integer sums are associative: the result does not depend on how the K branches are spread over lanes, waves and workgroups.
 *   6 outputs       plan [H, n, 8] float32, REQUIRED: the mean after the last iteration; it may be the pointer `mean` itself (the in-place call), any other overlap of
 *                   the two arrays is refused.  ret [K, n] float64, REQUIRED: the last iteration's returns on exit.  ret0 NULL or [iterations, n] float64: the
 *                   return of the plan entering each iteration (branch 0).  best_ret NULL or [n] float64: beta of the last iteration.  best_k NULL or [n] int32:
 *                   the smallest k attaining it (earl_minitaur_plan_candidates recovers that candidate).  fail NULL or [K, n] int32: the last iteration's count of
 *                   rolled-back steps per branch (earl_minitaur_branch_rollout's `fail`).
 *   7 non-finite    clip() maps a NaN of `mean` to -1 and +-Inf to +-1, so every candidate is finite whatever `mean` holds.  A NaN return never wins: beta is the
 *                   largest return that is not NaN, -Inf if there is none; x_k that is NaN (a NaN return, or Inf - Inf) gives W_k = 0; if S == 0 (no branch has a
 *                   weight) the update is skipped, mean' = m.  best_k is the smallest k with ret[k] == beta when beta > -Inf, and 0 otherwise.  Nothing of this faults.
 *   chaining        `iterations` iterations in one call equal that many calls with iterations = 1 and iteration0 = j, each fed the previous plan, bit for bit.
 *   determinism     the noise depends on (seed, global env id, j, k, t, noise_counter) only and the sums are integer: the plan is bit-identical across shard splits,
 *                   launch forms and graph replays.
 *   state           `st` is read and never written, as in the branch launch: the env is as earl_minitaur_branch_rollout leaves it.
 *   ws              ONE block as earl_minitaur_branch_ws describes it, of at least earl_minitaur_plan_ws_bytes(K, H, n, &bytes) bytes: the branch launch's workspace
 *                   and behind it the [K, H, n, 8] candidates of the current iteration at the next 16-byte address (the call aligns them itself).  The size is
 *                   monotone in K, H and n and 0 for K n == 0.  The caller prepares nothing in it and nothing in it outlives the call.
 * EARL_ERR_ARG before any HIP call, with a message in earl_last_error, for: everything earl_minitaur_branch_rollout refuses in model / col / cfg / st; params, mean, plan,
 * ret or ws NULL; K outside 1 .. EARL_MINITAUR_PLAN_MAX_K (one env's integer weights are held in 32 KB of LDS); H outside 1 .. 65536; iterations < 1, iteration0 < 0,
 * iteration0 + iterations > 256; a sigma that is negative or not finite; an inv_temperature that is not finite or <= 0; plan overlapping mean without being equal to it;
 * K * n beyond 2^31 - 1; with n > 0 a ws block that is NULL, misaligned (8 bytes) or too small.  n == 0 returns EARL_OK, launches nothing and writes nothing.  Under
 * earl_debug_set_minitaur_stepper(0) the call returns EARL_ERR_ARG, as the branch launch does. */
typedef struct earl_minitaur_plan_params {
  int32_t K;               /* candidates per env, branch 0 (the plan itself) included: 1 .. EARL_MINITAUR_PLAN_MAX_K */
  int32_t H;               /* steps of a plan: 1 .. 65536 */
  int32_t iterations;      /* I >= 1 */
  int32_t iteration0;      /* index of the first iteration (a word of the noise counter): >= 0, iteration0 + iterations <= 256 */
  float sigma[8];          /* noise scale per action dimension, finite, >= 0 */
  uint32_t noise_counter;  /* a word of the noise counter: a fresh value per control step gives fresh noise */
  double inv_temperature;  /* 1 / lambda, finite, > 0 */
} earl_minitaur_plan_params;
#define EARL_MINITAUR_PLAN_MAX_K 8192
/* *bytes = the size of the workspace of a planner call; EARL_ERR_ARG for bytes == NULL, K < 0, H < 0, n < 0, K * n beyond 2^31 - 1 */
int earl_minitaur_plan_ws_bytes(int32_t K, int32_t H, int32_t n, int64_t* bytes);
int earl_minitaur_plan_mppi(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                            const earl_minitaur_plan_params* params, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                            int32_t* fail, const uint64_t* clock, const earl_minitaur_branch_ws* ws, earl_stream_t stream);
/* Item 2 written out for ONE iteration j (0 .. 255): act_out [K, H, n, 8] float32, 16-byte aligned, what earl_minitaur_branch_rollout takes; earl_minitaur_plan_mppi runs
 * the same kernel.  It reads cfg->n, env_offset and seed and params->K, H, sigma and noise_counter only (no env state, no model).
 * EARL_ERR_ARG for cfg, params, mean or act_out NULL, act_out misaligned, n < 0, K or H out of range, j outside 0 .. 255, a bad sigma, K * n beyond 2^31 - 1; n == 0
 * returns EARL_OK and writes nothing. */
int earl_minitaur_plan_candidates(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream);
/* Host twins of the planner's own arithmetic (libearl_host.so; host pointers; csrc/minitaur_plan.h in plain loops -- there is no host stepper, so the scores are the
 * caller's).  earl_minitaur_plan_candidates_cpu: the call above (no alignment asked of act_out).  earl_minitaur_plan_update_cpu: items 4 - 7 of iteration j on GIVEN
 * candidates act [K, H, n, 8] and returns ret [K, n] -> plan [H, n, 8] (may be `mean`), and ret0_row / best_ret / best_k, each NULL or [n].  It reads cfg->n and
 * params->K, H and inv_temperature; its refusals are the planner's for those, for j and for the pointers. */
int32_t earl_minitaur_plan_candidates_cpu(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, float* act_out);
int32_t earl_minitaur_plan_update_cpu(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, const float* act, const double* ret,
                                      float* plan, double* ret0_row, double* best_ret, int32_t* best_k);

/* reset the envs with mask[i] != 0 (NULL = all); obs [n, 32] (may be NULL) is written for the reset envs only */
int earl_minitaur_reset(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                        const uint8_t* mask, double* obs, earl_stream_t stream);
int earl_minitaur_cfg_size(void);
/* measurement / test switch for the minitaur kernels: 1 (default) = the timestep written on the model's tree (csrc/minitaur_stepper.h: arrow-shaped
 * constraint Hessian eliminated legs -> root body, parent / child exchanges by DPP), 0 = the generic nv = 22 instantiation of the stepper (dense
 * factorisation).  Same algorithm; results agree to rounding (tests/test_minitaur_gpu.py). */
int earl_debug_set_minitaur_stepper(int tree);
/* The minitaur's fused rollout in its two-waves-per-SIMD form (csrc/physics_env_minitaur.h minitaur_duo_kernel: a timestep in two halves run by two waves; same results):
 * 1 = every packed launch, 0 = never, -1 = by batch size (the default).  Returns the previous setting.  Measurement / test switch. */
int earl_debug_set_minitaur_duo(int mode);
/* Small batches of the kitchen / minitaur launches (round 5; BASELINE configs[3] / [4] shard 2048 / 4096 envs over 8 GPUs: 256 / 512 per GPU).  An env is a serial chain of
 * T x frame_skip timesteps walked by one 32-lane group; the launch lasts as long as its slowest wave, and a wave's two envs wait for each other's longer branch in every
 * timestep.  -1 (default) = by batch size: n <= CUs: one env per WORKGROUP -- the kitchen with all FOUR waves on the env (mode 3: a timestep's constraint rows, mass matrix,
 * bias forces and collision phases side by side on the CU's four SIMDs, then one wave's active set and integration; csrc/physics_env_kitchen.h), the minitaur with one; n <= 4 x CUs:
 * one env per WAVE (the second group shadows the first one's env and stores nothing) -- the kitchen, for n <= 2 x CUs, with TWO waves per env, two envs per workgroup (mode 4: the
 * owner wave runs collision, rows, active set and integration, its helper the mass matrix, bias forces, equality Hessian and the integration's factor); otherwise two envs per wave.
 * 0 / 1 / 2 force a mode (2 = one env per workgroup, one wave), 3 / 4 (kitchen only) force the four-wave / two-wave form.  Results are bit-identical in every mode
 * (tests/test_kitchen_gpu.py, tests/test_minitaur_gpu.py).  earl_debug_set_solo: kitchen launches; earl_debug_set_solo_mt: minitaur launches.  Returns the previous setting. */
int earl_debug_set_solo(int mode);
int earl_debug_set_solo_mt(int mode);

/* measurement / test switch for the door model's rollout: 0 (default) = by batch size (n > 4096: one eight-wave workgroup per CU, see
 * csrc/physics_w8.hip; otherwise four single-wave workgroups per CU), 1 / 2 force the one or the other, 3 = single-wave workgroups under the time-sliced work
 * queue of the peg (needs earl_sawyer_state.sched; slower than 2 at N = 8192, tools/bench_door_schedule.py).  Results are bit-identical. */
int earl_debug_set_door_variant(int variant);
/* measurement / test switch for the peg model's rollout: 1 (default) = time-sliced schedule when earl_sawyer_state.sched is given and the batch exceeds one round,
 * 0 = always one group per wave, k >= 2 = time-sliced with k env steps per work item.  Results are bit-identical. */
int earl_debug_set_peg_schedule(int sliced);
/* measurement / test switch for the launch shape of the policy-prior branches (earl_sawyer_branch_rollout_prior and the `_prior` planners): 1 (default) = ONE launch of the
 * prior kernel over all K n virtual envs, the branches in front of K - P loading their action inside it; 2 = the untouched branch kernels over the first (K - P) n, then
 * the prior kernel over the last P n.  Results are bit-identical. */
int earl_debug_set_sawyer_prior_launches(int launches);

/* sizeof(earl_link_model) as compiled into the library (bindings check their struct layout against it) */
int earl_physics_model_size(void);
int earl_physics_model24_size(void);
int earl_collision_model_size(void);
int earl_sawyer_cfg_size(void);

#ifdef __cplusplus
}
#endif
#endif
