/*
 * ses.h -- C ABI of libses_hip.so, the MI355X (gfx950) implementation of the simple-es
 * population rollout + fitness hot path.
 *
 * The reference (jinPrelude/simple-es) is pure Python and has no FFI of its own; its seam is
 *     results = p.map(RolloutWorker, arguments)                 learning_strategies/evolution/loop.py:66-79
 *     offsprings, best, sigma = strategy.evaluate(results)      learning_strategies/evolution/loop.py:82-84
 * Every entry point below names the reference code it replaces.  The Python host
 * (simple-es_amd/ses/_lib.py) binds them with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.
 *   - every array argument is a CALLER-OWNED DEVICE pointer (e.g. torch tensor .data_ptr());
 *     the library never frees or reallocates it.  The handle owns only scratch.
 *   - calls enqueue work on the handle's HIP stream and return immediately; ses_sync() blocks.
 *   - a handle is bound to one device and one stream and is NOT thread-safe: use it from one host thread at a
 *     time (one handle per rank / per stream).  Calls may allocate handle-owned scratch on first use or when a
 *     larger population arrives, so they are not hipGraph-capturable until the sizes have been seen once.
 *   - return value: SES_OK (0) or a negative SES_ERR_*; ses_last_error() gives a message
 *     (thread-local).  No C++ exception crosses the boundary.
 *   - "row" = one offspring's flat parameter vector, float32[P], in torch parameters() order
 *     (networks/neural_network.py:46-56): fc1.weight(32,S) fc1.bias(32)
 *     [gru.weight_ih(96,32) gru.weight_hh(96,32) gru.bias_ih(96) gru.bias_hh(96)]
 *     fc2.weight(A,32) fc2.bias(A).
 *   - results are index-ordered like Pool.map: fitness[i] belongs to row i.
 */
#ifndef SES_H_
#define SES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SES_OK 0
#define SES_ERR_INVALID_ARG (-1)
#define SES_ERR_UNSUPPORTED (-2)
#define SES_ERR_HIP (-3)
#define SES_ERR_NO_DEVICE (-4)
#define SES_ERR_COMM (-5) /* RCCL not loadable, or a communicator call failed */

#define SES_HIDDEN 32 /* hidden width, hard-coded in networks/neural_network.py:12-17 */

/* env_id */
#define SES_ENV_NONE (-1)  /* no env: handle only serves policy-forward / strategy kernels */
#define SES_ENV_CARTPOLE 0 /* CartPole-v1 via envs/gym_wrapper.py:7-54 (conf/cartpole.yaml) */
#define SES_ENV_LUNARLANDER 1 /* LunarLanderContinuous-v2 via envs/gym_wrapper.py (conf/lunarlander_openai.yaml): gym's env     */
                              /* restated on a Box2D-style world (csrc/ses_lander.h, ses_b2.h + ses_b2_toi.h: discrete solver  */
                              /* and time-of-impact sub-stepping against the terrain; parity with gym / Box2D is              */
                              /* UNPINNED, neither is in the reference tree); num_state 8, num_action 4, continuous;        */
                              /* pomdp zeroes obs 2,3,5 (LunarLanderPOMDP, gym_wrapper.py:57-66); init rows: 16 uniforms.  */
                              /* discrete_action = 1 selects LunarLander-v2, gym's discrete lander on the same world step  */
                              /* (csrc/ses_lander_discrete.hip): argmax over the 4 outputs, first maximum wins; 0 = no-op, */
                              /* 1 = left engine, 2 = main engine, 3 = right engine = the continuous env's inputs (0, 0),  */
                              /* (0, -1), (1, 0), (0, +1), exactly; everything else as the continuous env                  */
#define SES_ENV_SIMPLE_SPREAD 2 /* pettingzoo MPE simple_spread via envs/pettingzoo_wrapper.py:6-64 (conf/simplespread.yaml); */
                                /* num_state = 6*n_agents, num_action = 5, discrete, MLP policy shared by the agents      */
#define SES_ENV_BIPEDALWALKER 3 /* BipedalWalker-v3 via envs/gym_wrapper.py (conf/bipedalwalker.yaml): gym's env restated on   */
                                /* the same Box2D-style world (csrc/ses_walker.h; parity UNPINNED); num_state 24, num_action  */
                                /* 4, continuous, MLP policy; init rows: 4 floats (force uniform, 2 terrain-key words, pad)   */
#define SES_ENV_ACROBOT 4 /* Acrobot-v1 via envs/gym_wrapper.py (conf/acrobot.yaml): gym 0.21's "book" dynamics restated in   */
                          /* float64 in gym's order of operations (csrc/ses_classic.h: RK4 over dt = 0.2, wrap, velocity  */
                          /* bounds; sin / cos without fma; parity with gym UNPINNED); num_state 6, num_action 3, discrete,*/
                          /* MLP or GRU policy, no pomdp, episodic only; init rows: 4 floats U(-0.1, 0.1) (theta1, theta2, */
                          /* dtheta1, dtheta2); state blob: the float64 state, 32 B; reward -1 per step, 0 on the terminal */
#define SES_ENV_MOUNTAINCAR 5 /* MountainCar-v0 via envs/gym_wrapper.py (conf/mountaincar.yaml): gym 0.21's env restated in    */
                              /* float64 (csrc/ses_classic.h; parity UNPINNED); num_state 2, num_action 3, discrete, MLP or */
                              /* GRU policy, no pomdp, episodic only; init rows: 1 float U(-0.6, -0.4) (position; velocity  */
                              /* 0); state blob: the float64 (position, velocity), 16 B; reward -1 per step                 */
#define SES_ENV_PENDULUM 6 /* Pendulum-v1 via envs/gym_wrapper.py (conf/pendulum.yaml): gym 0.21's env restated in float64   */
                           /* (csrc/ses_classic.h, equations in DESIGN.md 7; parity UNPINNED); num_state 3, num_action 1,    */
                           /* continuous (the tanh head; the env clips the torque to +-2), MLP or GRU policy, no pomdp,      */
                           /* episodic only; init rows: 2 floats U(-1, 1) (theta = u0 * pi, dtheta = u1); state blob: the    */
                           /* float64 (theta, dtheta), 16 B; reward = -(angle^2 + 0.1 dtheta^2 + 0.001 u^2) in float64;      */
                           /* never terminates: every episode is max_step steps                                             */
#define SES_ENV_MOUNTAINCAR_CONT 7 /* MountainCarContinuous-v0 via envs/gym_wrapper.py (conf/mountaincar_continuous.yaml): gym  */
                                   /* 0.21's env restated in float64 on a float32-rounded state (csrc/ses_classic.h;         */
                                   /* parity UNPINNED); num_state 2, num_action 1, continuous (the env clips the force to    */
                                   /* +-1), MLP or GRU policy, no pomdp, episodic only; init rows: 1 float U(-0.6, -0.4);    */
                                   /* state blob: the float64 (position, velocity), 16 B; reward = (100 at the goal) - 0.1   */
                                   /* a^2 of the UNclipped action, in float64                                               */
#define SES_ENV_WATERWORLD 8 /* waterworld via envs/pettingzoo_wrapper.py (conf/waterworld.yaml): the build's own float64         */
                             /* definition modelled on pettingzoo's sisl waterworld_v3 with its defaults (csrc/ses_waterworld.h,  */
                             /* DESIGN.md 7 is the specification; parity with pettingzoo UNPINNED); n_agents 5 (the pursuers),  */
                             /* num_state 242, num_action 2, continuous (the head's tanh output times 0.001f, as the reference  */
                             /* wrapper scales it), MLP policy shared by the pursuers, no GRU, no pomdp, episodic only; init    */
                             /* rows: 72 floats U(0, 1) (positions, headings, two key words of the env's respawn stream); never */
                             /* terminates: every episode is min(max_step, 500) cycles; eval_ep_num 1 .. 16                     */
#define SES_ENV_INVERTED_PENDULUM 9 /* InvertedPendulumBulletEnv-v0 via envs/gym_wrapper.py (conf/inverted_pendulum.yaml): the       */
                                    /* build's own float64 definition modelled on pybullet_envs (csrc/ses_pendula.h, DESIGN.md 7  */
                                    /* is the specification; parity with Bullet UNPINNED): a uniform rod hinged on a cart on a    */
                                    /* rail |x| <= 1, semi-implicit Euler at dt 0.0165; num_state 5, num_action 1, continuous    */
                                    /* (the tanh head; the env clips to +-1, force 100 a), MLP or GRU policy, no pomdp, no       */
                                    /* physics64, episodic only; init rows: 1 float U(-0.1, 0.1) (theta; all else 0); state blob: */
                                    /* the float64 (x, v, theta, omega), 32 B; reward 1 per step; done when |theta| > 0.2        */
#define SES_ENV_PENDULUM_SWINGUP 10 /* InvertedPendulumSwingupBulletEnv-v0 (conf/pendulum_swingup*.yaml): the same cart and rod   */
                                    /* (csrc/ses_pendula.h; parity UNPINNED), reset hanging: theta = 3.1415 + u; shapes, policies */
                                    /* and state blob as above; reward = cos theta of the new angle, in float64; never           */
                                    /* terminates: every episode is max_step steps                                                */
#define SES_ENV_DOUBLE_PENDULUM 11 /* InvertedDoublePendulumBulletEnv-v0 (conf/double_pendulum.yaml): two uniform rods on the     */
                                   /* cart (csrc/ses_pendula.h, the mass matrix and its solve in DESIGN.md 7; parity UNPINNED);  */
                                   /* num_state 9, num_action 1, continuous (force 200 a), MLP or GRU policy, no pomdp, no       */
                                   /* physics64, episodic only; init rows: 2 floats U(-0.1, 0.1) (theta1, theta2); state blob:   */
                                   /* the float64 (x, v, theta1, omega1, theta2, omega2), 48 B; reward = 10 - 0.01 x2^2 -        */
                                   /* (y2 + 0.3 - 2)^2 of the new state, in float64; done when y2 + 0.3 <= 1                     */
#define SES_ENV_PURSUIT 12 /* pursuit via envs/pettingzoo_wrapper.py (conf/pursuit.yaml): the build's own integer definition       */
                           /* modelled on pettingzoo's sisl pursuit_v3 with its defaults (csrc/ses_pursuit.h, DESIGN.md 7 is the   */
                           /* specification; parity with pettingzoo UNPINNED): 8 pursuers and 30 randomly moving evaders on a     */
                           /* 16 x 16 grid round one block; n_agents 8, num_state 147 (the pursuer's 7 x 7 x 3 window),           */
                           /* num_action 5, discrete (0 = x - 1, 1 = x + 1, 2 = y + 1, 3 = y - 1, 4 or anything else = stay),     */
                           /* MLP policy shared by the pursuers, no GRU, no pomdp, no physics64, episodic only; init rows: 40     */
                           /* floats U(0, 1): 8 pursuer cells, 30 evader cells (cell = free[min(192, (int)(u * 193.0f))] of the   */
                           /* 193 free cells in ascending (x, y) order; an evader with a negative entry does not exist), two key  */
                           /* words of the evader-move stream; done when no evader is left, else min(max_step, 500) cycles;       */
                           /* eval_ep_num 1 .. 16                                                                                   */
#define SES_ENV_REACHER 13 /* ReacherBulletEnv-v0 via envs/gym_wrapper.py (conf/reacher.yaml; the reference's envs/gym_wrapper.py:1-2  */
                           /* imports pybullet_envs): the build's own float64 definition modelled on pybullet's Reacher            */
                           /* (csrc/ses_reacher.h, DESIGN.md 7 is the specification; parity with Bullet UNPINNED): a planar arm of  */
                           /* two uniform rods, no gravity, semi-implicit Euler at dt 0.0165, elbow limited to |g| <= 3; num_state */
                           /* 9, num_action 2, continuous (two tanh heads; the env clips to +-1, torque 0.05 a per joint), MLP or  */
                           /* GRU policy, no pomdp, no physics64, episodic only; init rows: 4 floats U(-1, 1): target = 0.27 (u0,  */
                           /* u1), theta = pi u2, g = 3 u3, rates 0; state blob: the float64 (theta, w1, g, w2, target x, target   */
                           /* y, potential), 56 B; reward = the potential difference -100 (d' - d) minus the action costs, in      */
                           /* float64; never terminates: every episode is max_step steps (the wrapper's time limit is 150)         */
#define SES_ENV_HOPPER 14  /* HopperBulletEnv-v0 via envs/gym_wrapper.py (conf/hopper.yaml): the build's own float32 definition of  */
                           /* a planar one-legged hopper modelled on pybullet_envs' (csrc/ses_hopper_env.h on the Box2D-style world */
                           /* of ses_b2.h, DESIGN.md 7 is the specification; parity with Bullet UNPINNED): torso, thigh, leg, foot  */
                           /* on three revolute joints with limits, the foot in friction contact with flat ground; one env step = 4 */
                           /* world steps of 0.0165 / 4 s; num_state 15, num_action 3, continuous (three tanh heads; the env clips  */
                           /* to +-1, torque 150 a per joint), MLP or GRU policy, no pomdp, no physics64, episodic only; init rows: */
                           /* 3 floats U(-0.1, 0.1): the joint angles (clipped into their limits), zero velocities; step-wise       */
                           /* action float32[n, 3] = (thigh, leg, foot); reward float32 = alive +-1 + progress - electricity -      */
                           /* joints at limit; done when the torso is below 0.8 m, pitched by 1 rad or more, or touches the ground  */
#define SES_ENV_WALKER2D 15 /* Walker2DBulletEnv-v0 via envs/gym_wrapper.py (conf/walker2d.yaml): the build's own float32 definition */
                           /* of a planar two-legged walker modelled on pybullet_envs' (csrc/ses_walker2d_env.h on the Box2D-style  */
                           /* world of ses_b2.h, DESIGN.md 7 is the specification; parity with Bullet UNPINNED): the hopper's leg   */
                           /* twice on one torso, seven bodies on six revolute joints with limits, both feet in friction contact    */
                           /* with flat ground, the legs do not collide; one env step = 4 world steps of 0.0165 / 4 s; num_state    */
                           /* 22, num_action 6, continuous (six tanh heads; the env clips to +-1, torque 40 a per joint), MLP or    */
                           /* GRU policy, no pomdp, no physics64, episodic only; init rows: 6 floats U(-0.1, 0.1): the joint angles */
                           /* (clipped into their limits), zero velocities; step-wise action float32[n, 6] = (thigh, leg, foot,     */
                           /* thigh_left, leg_left, foot_left); reward and done as the hopper's, the means over six joints          */
#define SES_ENV_BIPEDALWALKER_HARDCORE 16 /* BipedalWalkerHardcore-v3 via envs/gym_wrapper.py (conf/bipedalwalker_hardcore.yaml): BipedalWalker-v3's */
                           /* body, observation, actions, reward and init row on a terrain of stumps, pits and stairs: one x-monotone */
                           /* polyline with vertical risers (csrc/ses_walker_hardcore_env.h, DESIGN.md 7 is the specification; the    */
                           /* build's own definition, parity with gym UNPINNED); num_state 24, num_action 4, continuous, MLP or GRU   */
                           /* policy, no pomdp, episodic only; init rows: 4 floats (force uniform, 2 terrain-key words, pad); step-   */
                           /* wise action float32[n, 4]; state blob: the env struct, then the terrain row of 2192 bytes               */

/* rollout / env-step mode */
#define SES_MODE_EPISODIC 0     /* an env stops at done (reference semantics, loop.py:116)      */
#define SES_MODE_FIXED_LENGTH 1 /* synthetic-benchmark mode: physics keeps stepping after done, */
                                /* rewards gated by the alive flag; identical returns            */

typedef struct ses_handle ses_handle;

typedef struct ses_config {
    int32_t env_id;          /* SES_ENV_*                                                        */
    int32_t num_state;       /* network.num_state   (conf/cartpole.yaml:7)                       */
    int32_t num_action;      /* network.num_action  (conf/cartpole.yaml:8)                       */
    int32_t discrete_action; /* network.discrete_action                                          */
    int32_t gru;             /* network.gru                                                      */
    int32_t pomdp;           /* env.pomdp: CartPolePOMDP zeroes obs[1], obs[3] (gym_wrapper.py:69-77) */
    int32_t max_step;        /* env.max_step (gym_wrapper.py:37-39); CartPole-v1 TimeLimit = 500 */
    int32_t eval_ep_num;     /* --eval-ep-num, run_es.py:33-38                                   */
    int32_t device;          /* HIP device ordinal                                               */
    int32_t lanes_per_env;   /* 0 = choose from the population size; else 1, 2, 4, 8, 16 or 32   */
    int32_t n_agents;        /* simple_spread: agents (= landmarks) per env, 2 (reference) or 3; else 1 */
    int32_t physics64;       /* CartPole rollouts only: 1 = gym-order float64 dynamics (csrc/ses_cartpole.h),   */
                             /* 0 = folded-constant fp32 (default, benchmark path)                              */
} ses_config;

/* ---- lifecycle --------------------------------------------------------------------------- */
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the
 * device's default stream. */
int ses_create(const ses_config *cfg, void *stream, ses_handle **out);
int ses_destroy(ses_handle *h);
int ses_sync(ses_handle *h);
/* Development / test hook: which of the (result-identical) rollout kernels a handle picks.  Every kernel evaluates the
 * same canonical arithmetic, so no setting changes a result; the defaults are the measured crossovers.  Knobs:
 * "gru_ep_parallel_max" (default 4096), "gru_mfma_min_e" (12), "gru_mfma4_min_e" (7; 0 = never | 1 ... 8: eval_ep_num from which -- up to 8 -- the CartPole GRU rollout takes its policy step on v_mfma_f32_4x4x1_16b_f32), "gru_sequential" (0), "rollout_mix" (1),
 * "rollout_waves8" (1024: light waves of the mixed CartPole MLP split), "rollout_mix_light" (their lanes per env: 0 = choose | 8 | 16), "rollout_lpe32_max_envs" (0: CartPole MLP populations of up to this many envs run at 32 lanes per env), "rollout_mix_8_16" (default 1: populations of 8193 ... ~12 000 envs run 8 lanes per env on every SIMD and the rest at 16), "rollout_handover_step" (2^30 = off: in fixed-length mode the (16, 4) mixed split runs as light + heavy wave pairs whose heavy wave hands half its envs to the light wave at this step, both finishing at 8 lanes per env | >= max_step: no hand-over), "rollout_heavy_prio_steps" (2^30 = all; 0 = none: steps for which the heavy wave of such a pair runs at s_setprio 1, so that VALU arbitration serves it before the older light wave), "rollout_packed" (-1: populations of at most one wave per SIMD run the packed form of the CartPole MLP step | 0: never | 1: whenever 8 or 16 lanes share an env), "rollout_heavy_packed" (-1: the launcher decides, which is 1 | 0: the heavy wave of such a pair runs the scalar step | 1: the packed one), "rollout_block" (64 | 256), "lander_offspring_per_wave" (0 = by population size | 1 | 2 | 4),
 * "box2d_lanes_per_env" (0 = by population size | 1 | 2 | ... | 64: lanes that share one env in the LunarLander / BipedalWalker MLP rollout),
 * "box2d_envs_per_wave" (0 = by population size | 1 ... 64 / lanes per env: different envs a wave of that rollout carries),
 * "pendulum_generic_step" (0 | 1: the Pendulum MLP rollout on the generic observe / step kernel instead of its own one-sincos kernel; A/B timing),
 * "reacher_generic_step" (-1: the default form, one-trig | 0: the Reacher MLP rollout evaluates the state's sin / cos once per step | 1: the generic observe / step form; same bits, A/B timing),
 * "pendula_generic_step" (-1: the form measured faster for the env | 0: the MLP rollout of the inverted-pendulum family evaluates each angle's sin / cos once per step | 1: the generic observe / step form; same bits, A/B timing),
 * "env_step_block" (64 | 128 | 256), "env_step_waves_per_cu" (1 ... 32, default 7) and "env_step_lds_bytes" (-1 ... 65536,
 * default -1): workgroup size of ses_env_step's kernel and the LDS each workgroup reserves without touching it -- -1 derives
 * the reservation from the device's LDS per CU so that env_step_waves_per_cu waves stay in flight (7 is what the memory
 * system wants; ses_env_step_shape reports what the occupancy calculator makes of it), >= 0 is taken as given,
 * "es_final_max_chunks" (0: ses_openai_generation applies Adam in its own small launch; k > 0: inside the gradient kernel for
 * populations of up to k * 1024 rows), "es_tail_wide" (default 1: the gradient kernel of the openai_es tail runs 1024-thread
 * workgroups, one row per thread; 0: the 256-thread form before it -- same bits, for measuring one against the other),
 * "comm_force_rccl" (1: ses_allgather_fitness uses the RCCL communicator although the
 * peer-store transport is attached -- for measuring one against the other), "comm_p2p_timeout_ms" (how long a peer-store
 * exchange waits for a peer's shard; 0 = default 60000), "comm_p2p_keep_going" (1: after a time-out later exchanges still
 * run instead of failing; the host polls ses_comm_p2p_status, agrees with the other ranks and rolls back -- ESLoop.run()),
 * "openai_sharded_tail" (default 1; 0: ses_openai_sharded_ok answers no, sharded runs keep the replicated openai_es tail),
 * "openai_sharded_min_rows" (default 8192: populations of fewer rows IN TOTAL keep the replicated tail -- the shard form costs a
 * second exchange and measured slower at 4096 rows in total),
 * "openai_granule_exchange" (default 1; 0: ses_openai_generation_sharded all-gathers its chunk partials with a launch of their
 * own also on the peer-store transport, as it does over RCCL -- for measuring one against the other),
 * "comm_granule_allgather" (default 0; 1: ses_allgather_fitness over the peer-store transport moves 8-byte {exchange number,
 * value} granules -- the data is its own flag -- while the shard fits half a mailbox section.  Measured slower for a whole
 * fitness shard, 12.4 us against 6.3 at 4096 floats; it is how a rank that does nothing else answers the granule exchange of
 * ses_openai_generation_sharded, tools/time_tail.py), "comm_granules_enabled" (default 1; 0: the handle's transport refuses
 * granule exchanges, the shard form of the tail then all-gathers its partials as floats), "fused_fitness_exchange" (default 1:
 * inside a sharded ses_run_generations above 8192 rows the fitness exchange needs no launch either -- the episode-mean kernel
 * stores every value as a granule into every rank's mailbox, the rank kernel polls the tiles it sorts; 0: ses_allgather_fitness
 * between rollout and tail), "fused_episode_mean" (default 1: ses_run_generations on one GPU, openai_es up to 8192 rows -- the
 * counting rank forms the episode means itself from the rollout's per-episode returns, no episode-mean launch; 0: as two launches),
 * "fused_elite_tail" (default 1: ses_run_generations on one GPU, simple_evolution / simple_genetic up to 512 rows -- episode mean,
 * rank, best reward and elite selection in one launch, simple_evolution's elite rows and their mean in a second; 0: seven launches),
 * "fused_apply_perturb" (default 1: ses_openai_generation, replicated form, policies up to 1024 parameters and populations up to
 * 16 384 rows -- every workgroup of the launch that writes the next population applies the Adam update itself; 0: a launch of its own),
 * "fused_perturb_rollout" (default 1: ses_run_generations on one GPU, openai_es with that fused launch, fixed-length CartPole MLP
 * populations that run as light + heavy wave pairs (16 385 ... 20 480 envs) with eval_ep_num >= 2 -- between two generations of one
 * call that launch is not made: every workgroup of the NEXT rollout applies the update and draws the rows its waves run, into LDS
 * and into the population, before its step loop; the call's last generation launches it as before; 0: launched every generation),
 * "pgpe_fused_apply_perturb" (default 1: ses_pgpe_generation, policies up to 1024 parameters and populations up to 32 768 rows -- every
 * workgroup of the launch that draws the next population applies the update of (mu, m, v, scale) itself; 0: a launch of its own;
 * bit-equal results),
 * "ars_fused_apply_perturb" (default 1: ses_ars_generation and ses_ars_generation_batch, policies up to 1024 parameters and up to 16 384 selected pairs -- every
 * workgroup of the launch that draws the next population applies the update of mu itself; 0: a launch of its own; bit-equal results),
 * "spread_gru_wave_per_batch" (simple_spread with the GRU policy, whose lockstep step advances 8 (episode, agent) columns = 4 envs of
 * two agents or 2 of three per batch: 0 = a wave plays the batches of its offspring one after the other, weights loaded once; 1 = one
 * wave per (offspring, batch), weights re-read per batch; default -1: 1 while offspring x batches stays within the measured crossover).
 "waterworld_fc1_mfma" (the waterworld rollout's 242-wide fc1: 1 = on v_mfma_f32_32x32x2_f32, 0 = the same k-ascending chain on
 * the VALU, same bits; default -1 = the form measured faster, profiles/waterworld_timing.txt).
 * "pursuit_fc1_mfma" (the pursuit rollout's 147-wide fc1, the same choice: 1 = v_mfma_f32_32x32x2_f32 over K padded to 148, 0 = the
 * VALU chain, same bits; default -1 = the form measured faster, profiles/pursuit_timing.txt).
 * The library itself reads no environment variable.
 * Names, defaults and ranges are DEFINED in one table, csrc/ses_tuning.h (struct Tuning and its knob rows), which ses_tuning_info
 * enumerates; the list above describes them. */
int ses_set_tuning(ses_handle *h, const char *name, int32_t value);
/* Row `index` (0, 1, ...) of that table: the knob's name (a static string), its default and its range [lo, hi].  Needs no device and
 * no handle.  Past the last row: SES_ERR_INVALID_ARG.  Any out pointer may be NULL. */
int ses_tuning_info(int32_t index, const char **name, int32_t *default_value, int32_t *lo, int32_t *hi);
/* Test hook: launches this handle has made since ses_create (any pointer may be NULL) -- rollouts by the light + heavy pair kernel
 * of the CartPole MLP policy in either form, those of them that formed their own rows ("fused_perturb_rollout"), and launches of
 * the kernel that applies the openai_es update and writes the next population. */
int ses_launch_counts(ses_handle *h, int64_t *pair_rollouts, int64_t *perturb_rollouts, int64_t *apply_perturb);
/* Timing without events: from now on the last kernel of every ses_rollout (the episode mean: end of the rollout phase)
 * and every perturbation launch (ses_perturb, ses_perturb_host_noise, ses_openai_generation: the next population is
 * being written) of this handle stores the GPU's constant-rate real-time counter (100 MHz, common to all kernels,
 * streams and handles of the device) into *dst -- device-visible memory, e.g. pinned host memory the caller polls.
 * NULL switches it off.  Replaces the HIP events around `p.map(RolloutWorker, ...)` / `strategy.evaluate` that
 * loop.py:64-86 times with time.time(): an event costs the launch stream ~4.7 us, a stamp nothing. */
int ses_set_stamp(ses_handle *h, uint64_t *dst);
const char *ses_last_error(void);
const char *ses_version(void);
/* number of parameters P of GymEnvModel(S, A, _, gru)  (networks/neural_network.py:9-18) */
int ses_param_count(int32_t num_state, int32_t num_action, int32_t gru);
/* number of visible HIP devices, or a negative error (never initialises a context) */
int ses_device_count(void);

/* What the library's env table (csrc/ses_env_table.h, one row per env_id) says about the env of a config.  Needs no device and no
 * handle, like ses_param_count: a host reads here what it would otherwise restate.  The config is checked as ses_create checks
 * the env's own fields (num_state, num_action, discrete_action, gru, pomdp, physics64, n_agents, the eval_ep_num cap), with the same
 * messages; SES_ENV_NONE and an id without a row are SES_ERR_INVALID_ARG.
 *   init_width, init_lo, init_hi  one initial-state row: init_width floats U(init_lo, init_hi)  (ses_init_states_uniform, ses_rollout)
 *   obs_width                     floats per env of ses_env_reset / ses_env_step_generic: num_state * agents
 *   state_bytes                   ses_env_state_bytes of a handle of this config
 *   action_layout, agents, num_action   the `action` of ses_env_step_generic: SES_ACTION_* below, n = envs
 *   has_ep_steps                  0: ses_rollout takes no ep_steps (episodes of one fixed length)
 *   is_f64                        1: one of the float64 control envs (ses_obs_norm_bind serves them) */
#define SES_ACTION_I32_N 0           /* int32[n]                        */
#define SES_ACTION_I32_N_AGENTS 1    /* int32[n, agents]                */
#define SES_ACTION_F32_N_A 2         /* float32[n, num_action]          */
#define SES_ACTION_F32_N_AGENTS_A 3  /* float32[n, agents, num_action]  */
struct ses_env_info {
    int32_t init_width, obs_width, state_bytes;
    int32_t action_layout, agents, num_action;
    int32_t has_ep_steps, is_f64;
    double init_lo, init_hi;
};
int ses_env_info(const ses_config *cfg, struct ses_env_info *out);

/* Test hook: the launch form ses_rollout would choose for n_rows offspring of this config under `mode` (SES_MODE_*) -- what the rules
 * of csrc/ses_rollout_plan.h answer, evaluated on the host.  Needs no device and no handle.  The knobs start at their defaults;
 * knob_names[i] = knob_values[i] (i < n_knobs; both may be NULL when n_knobs is 0) override them, checked as ses_set_tuning checks
 * them.  The config is checked as ses_env_info checks it.  Every kernel form computes the same bits: the plan says which one runs.
 *   family                    SES_PLAN_* below; SES_PLAN_OTHER (the float64 envs, simple_spread, waterworld, pursuit: their forms are
 *                             chosen in their own units) leaves every other field 0
 *   lanes_light, lanes_rest   CartPole MLP, lanes per env: PURE, F64 -- of every wave, in lanes_rest; MIX, PAIR -- of the first
 *                             waves_light waves and of the waves_rest that follow
 *   handover                  PAIR: the step at which the heavy wave hands half its envs over (>= max_step: never)
 *   packed, block             PURE: the packed form of the step; threads per workgroup
 *   heavy_packed              PAIR: the packed form of the step in the heavy wave
 *   own_rows_ok               PAIR: inside ses_run_generations the rollout may form its own rows ("fused_perturb_rollout")
 *   gru_form                  GRU: SES_GRU_FORM_* below
 *   box2d_lpe, box2d_epw      BOX2D_MLP: lanes per env, different envs per wave */
#define SES_PLAN_OTHER 0
#define SES_PLAN_CARTPOLE_MLP_PURE 1
#define SES_PLAN_CARTPOLE_MLP_MIX 2
#define SES_PLAN_CARTPOLE_MLP_PAIR 3
#define SES_PLAN_CARTPOLE_MLP_F64 4
#define SES_PLAN_GRU 5
#define SES_PLAN_BOX2D_MLP 6
#define SES_GRU_FORM_SEQUENTIAL 0
#define SES_GRU_FORM_EPISODE_PARALLEL 1
#define SES_GRU_FORM_MFMA4 2
#define SES_GRU_FORM_MFMA 3
#define SES_GRU_FORM_LOCKSTEP_MULTI4 4
#define SES_GRU_FORM_LOCKSTEP_MULTI2 5
#define SES_GRU_FORM_LOCKSTEP 6
struct ses_rollout_plan_info {
    int32_t family;
    int32_t lanes_light, lanes_rest, waves_light, waves_rest, handover;
    int32_t packed, heavy_packed, block, own_rows_ok;
    int32_t gru_form;
    int32_t box2d_lpe, box2d_epw;
};
int ses_rollout_plan(const ses_config *cfg, const char *const *knob_names, const int32_t *knob_values, int32_t n_knobs, int32_t n_rows,
                     int32_t mode, struct ses_rollout_plan_info *out);

/* ---- K1: offspring perturbation ---------------------------------------------------------- */
/*
 * theta[i,:] = parents[k,:] + sigma * eps(seed, gen, row_i, :)   if parent_idx[i] = k >= 0
 * theta[i,:] = parents[k,:]                                      if parent_idx[i] = -1-k
 * row_i = row_ids ? row_ids[i] : first_row + i   (GLOBAL offspring index: the noise is a pure
 * function of (seed, gen, row, column), so any shard of any GPU count reproduces the same rows).
 * eps: rocRAND Philox4x32-10 device engine + deterministic Box-Muller.
 * Replaces the deepcopy + np.random.normal loops of offspring_strategies.py:53-60 (simple_genetic),
 * :169-176 (simple_evolution), :312-326 (openai_es).  parent_idx == NULL: every row perturbs parent 0.
 */
int ses_perturb(ses_handle *h, const float *parents, const int32_t *parent_idx, const int32_t *row_ids,
                float sigma, uint64_t seed, uint64_t gen, int64_t first_row, int32_t n_rows, float *theta);
/* the raw normals eps[n_rows, P] of the same stream (tests, diagnostics) */
int ses_noise(ses_handle *h, uint64_t seed, uint64_t gen, int64_t first_row, int32_t n_rows, float *eps);
/*
 * Reference-stream mode: eps64[n_rows,P] are float64 normals drawn on the host from the
 * reference's own generator (np.random.normal, offspring_strategies.py:57,173,320) and uploaded.
 *   theta[i,:]        = (float)( (double)parent + eps64 * sigma )   -- offspring_strategies.py:322
 *   eps_store[i,:]    = (float)( (double)parent + eps64 )           -- :321 (openai_es.epsilons quirk,
 *                        SURVEY 3.4-4); may be NULL
 * bit-identical to the reference's float64-then-float32 arithmetic.  np.random.normal(0, sigma) of
 * :57/:173 is sigma * z on the same gauss stream, so the host always uploads standard normals z.
 */
int ses_perturb_host_noise(ses_handle *h, const float *parents, const int32_t *parent_idx,
                           const double *eps64, double sigma, int32_t n_rows, float *theta,
                           float *eps_store);
/* Reset distribution U(lo,hi)^width from the ENV_INIT Philox stream, out[n_rows,E,width]
 * (CartPole: width 4, U(-0.05,0.05); simple_spread: width 4*n_agents = agent then landmark positions,
 * U(-1,1); waterworld: width 72, U(0,1); pursuit: width 40, U(0,1)); width <= 72.  The counter of a draw is (row, episode * 8 + quad of the row), so rows wider
 * than 32 floats share draws with the next episodes' rows of the same offspring (waterworld: different but not independent episodes).
 * shared != 0 keys every row as offspring 0 (common random numbers).  The reference never
 * seeds its env: initial states are an explicit input of this library. */
int ses_init_states_uniform(ses_handle *h, uint64_t seed, uint64_t gen, int64_t first_row, int32_t n_rows,
                            int32_t shared, int32_t width, float lo, float hi, float *out);
/* The same for `gens` consecutive generations in ONE launch: out[g, n_rows, E, width] = what ses_init_states_uniform writes
 * for generation gen0 + g.  The resets depend on (seed, generation, row) only, so a generation loop draws them a chunk
 * ahead instead of once per generation (ESLoop.rollout, ses_run_generations). */
int ses_init_states_uniform_gens(ses_handle *h, uint64_t seed, uint64_t gen0, int32_t gens, int64_t first_row,
                                 int32_t n_rows, int32_t shared, int32_t width, float lo, float hi, float *out);

/* ---- K2: population-batched policy forward (networks/neural_network.py:20-36) ------------- */
/* n independent (row, observation[, hidden]) triples.  hidden: float32[n,32] in/out, NULL for MLP.
 * logits[n,A]: fc2 pre-activation; act[n,A] (may be NULL): tanh(logits), the continuous action;
 * action[n]: argmax(logits), first maximum wins (== torch.argmax(softmax) up to fp ties).
 * obs is the observation THE POLICY SEES: a caller that plays a policy trained with the observation normaliser below
 * normalises first (GymEnvModel.forward does); this entry point applies none. */
int ses_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int32_t n,
                       float *logits, float *act, int32_t *action);

/* ---- the running observation normaliser of ARS V2 (Mania, Guy & Recht 2018, Algorithm 2) ----
 * An opt-in for MLP policies on the eight float64 envs (Acrobot-v1, MountainCar-v0, Pendulum-v1, MountainCarContinuous-v0, the
 * three inverted pendulums, ReacherBulletEnv-v0), with every strategy.  State, caller-owned device buffers:
 *   stats   float64[S, 3]   row k = (n, mean_k, M2_k); the count is repeated per component (components merge independently)
 *   affine  float32[2, S]   shift[k], then scale[k]
 * Fresh state: n = mean = M2 = 0, shift = 0, scale = 1.
 * ses_obs_norm_bind binds them to the handle: from then on every ses_rollout of the handle, those that ses_run_generations issues
 * included, shows the policy on[k] = fl(fl(obs[k] - shift[k]) * scale[k]) (float32, one rounding per operation; shift and
 * scale are read once before the step loop) instead of obs[k] -- with the fresh state that is obs[k] bit for bit.  Physics,
 * rewards, termination and returns are untouched.  update != 0: the rollout also sums, per env and in step order, the RAW
 * observation that produced each action that was taken, and its square, in float64 (a frozen or finished env adds nothing,
 * nor does the observation after the last step); one more launch between the rollout kernel and the episode mean reduces
 * them over the envs in an order that is a function of the env count alone (lane l of 256 adds envs l, l + 256, ... ascending
 * from +0.0; then x[l] += x[l + s] for s = 128 ... 1; no floating-point atomics) and merges batch (n_b, S1, S2) into component k:
 *   n_b == 0: nothing is written.   mb = S1 / n_b;  M2b = max(S2 - S1 mb, 0);  N = n + n_b;  f = n_b / N;  d = mb - mean;
 *   mean += d f;  M2 = (M2 + M2b) + (d d)(n f);  n = N;  std = sqrt(M2 / (N - 1)) (N >= 2, else 1);
 *   shift[k] = (float)mean;  scale[k] = std < 1e-7 ? 0 : (float)(1 / std)       (scale 0: ARS's std = inf for a constant component)
 * every float64 operation rounded once.  The next rollout on the stream reads the affine this merge wrote: stream order only.
 * update == 0 normalises without accumulating or merging (evaluation, playback).  stats == NULL unbinds.
 * SES_ERR_UNSUPPORTED, the message naming the reason: an env that is not one of the eight, a GRU handle, a handle with a
 * communicator of world > 1 (the statistics would need an exchange). */
int ses_obs_norm_bind(ses_handle *h, double *stats, float *affine, int32_t update);
/* The reduction and merge alone, on caller-made partials float64[2 S + 1, n_env] (row 0: the envs' step counts, rows 1 .. S: the
 * sums s1[k], rows S + 1 .. 2 S: the sums of squares s2[k]) -- the layout the rollout leaves in the handle's scratch.  S is the
 * handle's env's observation width; the handle needs one of the eight envs. */
int ses_obs_norm_merge(ses_handle *h, const double *partials, int32_t n_env, double *stats, float *affine);

/* ---- K3: SoA env step (envs/gym_wrapper.py:32-45 around the third-party gym physics) ------- */
/* CartPole, one lane = one env, fp32 state in structure-of-arrays form.
 * status[i]: bits 0..30 steps taken, bit 31 done.  ret[i] += 1 per live step.
 * Algorithmic traffic 52 B / env-step: loads x,xd,th,thd,action,ret,status; stores all but action.
 * States are saturated at |x|, |xd|, |thd| <= 1e4 and |th| <= 0.75 rad: past-terminal values only (an episode ends
 * at |x| > 2.4 or |th| > 0.2095), which matter in SES_MODE_FIXED_LENGTH where finished envs keep stepping. */
int ses_env_step(ses_handle *h, int32_t n, int32_t mode, float *x, float *xd, float *th, float *thd,
                 const int32_t *action, float *ret, uint32_t *status);

/* ---- step-wise env entry for every env (envs/gym_wrapper.py:23-45, envs/pettingzoo_wrapper.py:22-58) ------------------ */
/* `env.reset()` / `env.step(action)` of the reference's wrappers for n independent envs, one lane = one env, through the
 * SAME device functions the fused rollouts call (csrc/ses_envs.hip).  The state of an env is an opaque blob of
 * ses_env_state_bytes(h) bytes in caller-owned device memory (CartPole 16 B; simple_spread 24 * n_agents + 4; LunarLander /
 * BipedalWalker: the Box2D-style world of the env followed by the episode's terrain heights; Acrobot / MountainCar /
 * Pendulum / MountainCarContinuous: the float64 state, 32 / 16 / 16 / 16 B; waterworld: position and velocity of its 20 objects in
 * float64, the two key words and the draw counter of its respawn stream, the ten touch flags; pursuit: 96 B -- the cells of the 8
 * pursuers and 30 evaders, one byte a coordinate, the mask of the live evaders, the two key words of the evader-move stream and
 * the cycle counter).
 *   ses_env_reset:  init[n, W] (W as for ses_rollout: CartPole 4, simple_spread 4 * n_agents, LunarLander 16, BipedalWalker 4,
 *                   Acrobot 4, MountainCar 1, Pendulum 2, MountainCarContinuous 1, waterworld 72, pursuit 40)
 *                   -> state[n], obs[n, ses_env_obs_width(h)]  (simple_spread: [n, n_agents, 6 * n_agents]; waterworld: [n, 5, 242]; pursuit: [n, 8, 147],
 *                   a window flattened [dx][dy][wall, pursuers in the cell, live evaders in the cell]); the Box2D envs
 *                   end their reset with gym's no-op step.
 *   ses_env_step_generic: action = int32[n] (CartPole, Acrobot, MountainCar: {0, 1, 2}, clamped into it; LunarLander with
 *                   discrete_action = 1: {0, 1, 2, 3}, any other value acts as 0, the no-op), int32[n, n_agents]
 *                   (simple_spread), float32[n, 5, 2] (waterworld: every pursuer's action ALREADY multiplied by 0.001f; reward = the
 *                   team reward of the cycle, its float64 value rounded to float; done is always 0), int32[n, 8] (pursuit: every
 *                   pursuer's move 0 .. 4, any other value stays; reward = the team reward of the cycle -- the eight equal shares of
 *                   the mean of the pursuers' own rewards, added up -- its float64 value rounded to float; done = no evader is left)
 *                   or float32[n, num_action]
 *                   (LunarLander with discrete_action = 0 uses components 0 and 1; BipedalWalker all four; Pendulum and
 *                   MountainCarContinuous float32[n, 1]: any float, the env clips it to +-2 / +-1 and never rejects it), already
 *                   in the env's action space (the policy's tanh output) -> obs, reward[n] (simple_spread: the team reward of the cycle,
 *                   pettingzoo_wrapper.py:45-52), done[n] = the ENV's own termination (CartPole: |x| > 2.4 or |th| > 12
 *                   deg; simple_spread: after 25 cycles; Box2D: crash / out of bounds / asleep; Acrobot: -cos th1 - cos(th2 + th1) > 1;
 *                   MountainCar: position >= 0.5 and velocity >= 0; Pendulum: never; MountainCarContinuous: position >= 0.45
 *                   and velocity >= 0).  The reward of Pendulum and MountainCarContinuous is their float64 reward rounded to
 *                   float (the fused rollouts add the float64 one).  Truncation at env.max_step is
 *                   the wrapper's (gym_wrapper.py:37-39).  POMDP handles zero the masked observation components
 *                   (gym_wrapper.py:57-77).  A finished env may be stepped on (its state keeps evolving); callers reset it. */
int ses_env_state_bytes(ses_handle *h);
int ses_env_obs_width(ses_handle *h);
int ses_env_reset(ses_handle *h, const float *init, int32_t n, void *state, float *obs);
int ses_env_step_generic(ses_handle *h, void *state, const void *action, int32_t n, float *obs, float *reward,
                         int32_t *done);

/* The launch shape ses_env_step (and ses_stream_probe) use on this device with the current knobs: threads per workgroup, the
 * LDS bytes each workgroup reserves, the waves per CU the HIP occupancy calculator gives that shape (0: unknown), and the
 * device's LDS per CU the default reservation is derived from.  Any pointer may be NULL. */
int ses_env_step_shape(ses_handle *h, int32_t *block, int32_t *lds_bytes, int32_t *waves_per_cu, int32_t *lds_per_cu);

/* ---- Rendering: `env.render()` of the reference's wrappers (envs/gym_wrapper.py:50-51, envs/pettingzoo_wrapper.py:63-64) and the
 * frames its test.py --save-gif collects (test.py:59-67), for n state blobs of the step-wise envs at once (csrc/ses_render.hip;
 * DESIGN.md section 19).  Two layers: a SCENE BUILDER per env turns a state blob into a short list of integer primitives, ONE
 * env-independent RASTERISER turns lists into palette-indexed frames.  The scenes are the build's own depictions, modelled on the
 * upstream renderers; pixel parity with gym / pettingzoo is not a goal.
 *
 * A frame is width x height bytes, each a palette index 0 .. 15, row 0 on top.  Coordinates are int32 in 1/16 PIXEL, origin at the
 * frame's top-left corner, x to the right, y DOWN; pixel (px, py) is sampled at p = (16 px + 8, 16 py + 8).  A primitive is
 * int32[8] = {kind, colour, x0, y0, x1, y1, x2, y2}; the colour used is colour & 15.  With cross(u, v) = u.x v.y - u.y v.x, over
 * EXACT integers, a sample is covered by
 *   SES_RENDER_TRI      v0, v1, v2: iff A = cross(v1 - v0, v2 - v0) != 0 and, s = sign(A), s cross(v1 - v0, p - v0) >= 0,
 *                       s cross(v2 - v1, p - v1) >= 0 and s cross(v0 - v2, p - v2) >= 0 (edges inclusive, both orientations draw);
 *   SES_RENDER_DISC     centre (x0, y0), r = x1: iff r >= 0 and |p - c|^2 <= r^2;
 *   SES_RENDER_CAPSULE  a = (x0, y0), b = (x1, y1), r = x2: iff r >= 0 and, d = b - a, L2 = |d|^2, t = d . (p - a): |p - a|^2 <= r^2
 *                       where t <= 0, |p - b|^2 <= r^2 where t >= L2, cross(d, p - a)^2 <= r^2 L2 in between;
 *   SES_RENDER_FILL     always;
 *   any other kind      never (the primitive is skipped).
 * Painter's order: a frame starts as index 0, the primitives of its list are applied in ascending index, later ones overwrite.
 * counts[i] above cap is read as cap (below 0: as 0).  Coordinates and radii are defined for [-16384, 16383]; a value outside it is
 * the caller's error and gives undefined pixels (this build does not draw such a primitive) -- never an access outside the
 * frame buffer, the kernel iterates over frame pixels only.
 *   ses_render_palette: the 16 RGB triples the indices stand for (host only; no handle).
 *   ses_render_size:    the nominal canvas of the handle's env (host only): 600 x 400 for CartPole, LunarLander and BipedalWalker,
 *                       400 x 400 for simple_spread.  Any other env: SES_ERR_UNSUPPORTED, the message names the ones that have a scene.
 *   ses_render_scene:   state[n] (blobs of ses_env_reset / ses_env_step_generic) -> prims[n, SES_RENDER_MAX_PRIMS, 8], counts[n]: one
 *                       lane per state, one launch.  A primitive whose bounding box lies wholly outside the canvas is dropped, the
 *                       coordinates of the others are clamped into the defined range.  Other envs: SES_ERR_UNSUPPORTED as above.
 *   ses_render_frames:  prims[n, cap, 8], counts[n] -> frames[n, height, width]: ONE launch for all n frames, for any handle (also
 *                       one created with SES_ENV_NONE).  1 <= width, height <= 1024, 1 <= cap <= SES_RENDER_MAX_PRIMS.
 * Neither launch synchronises the device. */
#define SES_RENDER_MAX_PRIMS 256
#define SES_RENDER_TRI 0
#define SES_RENDER_DISC 1
#define SES_RENDER_CAPSULE 2
#define SES_RENDER_FILL 3
int ses_render_palette(uint8_t *rgb /* [48] */);
int ses_render_size(ses_handle *h, int32_t *width, int32_t *height);
int ses_render_scene(ses_handle *h, const void *state, int32_t n, int32_t *prims, int32_t *counts);
int ses_render_frames(ses_handle *h, const int32_t *prims, const int32_t *counts, int32_t n, int32_t cap, int32_t width,
                      int32_t height, uint8_t *frames);

/* Measurement aid for the roofline of ses_env_step (no reference counterpart): the same 13 streams -- 7 x 16-byte
 * non-temporal loads and 6 x 16-byte non-temporal stores per lane over the same arrays, same grid -- with no arithmetic
 * in between; every value is written back unchanged.  Its duration is what the memory system of the box gives this
 * access pattern; bench.py prints it next to the env-step kernel's (roofline.copy13_*).  n a multiple of 4, arrays
 * 16-byte aligned. */
int ses_stream_probe(ses_handle *h, int32_t n, float *x, float *xd, float *th, float *thd, const int32_t *action,
                     float *ret, uint32_t *status);

/* ---- fused rollout: RolloutWorker for the whole shard (loop.py:108-125) -------------------- */
/*
 * theta[n_rows,P]; init: float32 [E,W] (init_per_offspring = 0, shared) or [n_rows,E,W], W = 4 for
 * CartPole (the state), 4*n_agents for simple_spread (agent positions, landmark positions), 4 for Acrobot, 1 for
 * MountainCar and MountainCarContinuous, 2 for Pendulum, 72 for waterworld (one wave per offspring and six episodes; the 242-wide
 * fc1 on the matrix cores or the VALU, "waterworld_fc1_mfma"; it adds the float64 team rewards), 40 for pursuit (one wave per offspring
 * and four episodes, "pursuit_fc1_mfma"; float64 team rewards added in cycle order; an episode ends when no evader is left).  The MLP rollouts of these four classic-control envs run at
 * lanes_per_env 1, 2, 4, 8, 16 or 32 (0: by population size); Pendulum and MountainCarContinuous add their float64 rewards.
 * fitness[n_rows] = sum over the E episodes of the undiscounted return / E  (loop.py:124).
 * ep_return (float64[n_rows,E]) and ep_steps (int32[n_rows,E]) may be NULL.
 * The whole episode loop (policy forward + env step, <= max_step iterations) runs inside one kernel
 * with env state, GRU state and the offspring's weights held in registers.
 */
int ses_rollout(ses_handle *h, const float *theta, const float *init, int32_t init_per_offspring,
                int32_t n_rows, int32_t mode, float *fitness, double *ep_return, int32_t *ep_steps);

/* ---- K4: rank-centred fitness shaping (offspring_strategies.py:380-398) --------------------- */
/* rank[i] = number of offspring that beat i (reward descending; ties: higher index first, i.e.
 * np.flip(np.argsort(kind="stable"))).  weights[i] = ((n-1-rank)/(n-1) - 0.5) / std, float64,
 * with the closed-form std sqrt((n+1)/(12(n-1))) of the rank grid.  weights may be NULL.
 * best (float32[1], may be NULL) receives the fitness of the offspring with rank 0, i.e. max(rewards): the
 * `best_reward` that evaluate() returns (offspring_strategies.py:420-434), so that the host reads one float back
 * instead of reducing the vector. */
int ses_rank_center(ses_handle *h, const float *fitness, int32_t n, int32_t *rank, double *weights, float *best);

/* ---- K5: ES gradient + Adam (offspring_strategies.py:400-416, optimizers.py:13-24,42-57) ---- */
/* One generation's fitness loop of openai_es (offspring_strategies.py:380-419 followed by _gen_offsprings :284-328) in
 * three launches (up to 8192 offspring): counting rank with the keys formed inline, ES-gradient partials with the
 * rank-centring weights formed inline and Adam applied by the last workgroup, Philox perturbation of the next population
 * (larger populations: keys, tile sort, search, gradient, update, perturbation).  Bit-identical to ses_rank_center +
 * ses_es_update_philox(skip_row0 = 1) + ses_perturb called one after the other (tests/test_gpu_host_mirror.py).
 *   fitness[n]: the gathered fitness of the evaluated population (noise generation `gen`, std `sigma`);
 *   (mu, m, v)_in -> (mu, m, v)_out: distinct float32[P] buffers, the caller ping-pongs them;
 *   theta_next[n_rows, P]: rows [first_row, first_row + n_rows) of the next population (noise generation next_gen, std
 *   next_sigma; global row 0 = the new mu itself); best: optional float32[1] <- max(fitness). */
int ses_openai_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double lr,
                          double sigma, double adam_a, const float *mu_in, const float *m_in, const float *v_in,
                          float *mu_out, float *m_out, float *v_out, float next_sigma, uint64_t next_gen,
                          int64_t first_row, int32_t n_rows, float *theta_next, float *best);
/* The same generation when the population is sharded over `world` ranks (loop.py:66-84 with one process per GPU) WITHOUT
 * every rank repeating the O(n) work: this rank ranks only its own rows [first_row, first_row + n_rows) against the gathered
 * fitness (n <= 8192: counting rank; above: every workgroup sorts one 1024-key tile and searches it for 1024 own rows) and
 * accumulates the ES gradient over its own 1024-row chunks only; the ranks then exchange their [chunks per rank, P] chunk
 * partials -- with the candidates for max(fitness) behind them -- through `comm`'s transport (58 KB in total at 65 536 x 226)
 * and the unchanged ordered update adds the chunks in ascending order.  On the peer-store transport the exchange needs no
 * launch: the gradient kernel stores every partial as one 8-byte {exchange number, value} granule straight into every rank's
 * mailbox and the update kernel polls the granules where they land (the data is the flag); over RCCL, or when a mailbox
 * section cannot hold the granules, the partials are all-gathered as floats by ses_allgather_fitness in between.
 * Bit-identical to ses_openai_generation for ANY world size, because a rank's slot of per_rank = ceil(n / world) rows is a
 * whole number of the gradient's 1024-row chunks -- that is the condition; ses_openai_sharded_ok tells (1 / 0) whether it
 * holds and `comm` (a handle on the same device and stream that owns a transport of `world` ranks which takes the payload)
 * can carry it.  Otherwise: SES_ERR_UNSUPPORTED, use ses_openai_generation.  Collective: every rank calls it. */
int ses_openai_sharded_ok(ses_handle *h, ses_handle *comm, int32_t n, int32_t per_rank, int32_t world);
int ses_openai_generation_sharded(ses_handle *h, ses_handle *comm, const float *fitness, int32_t n, uint64_t seed, uint64_t gen,
                                  double lr, double sigma, double adam_a, const float *mu_in, const float *m_in,
                                  const float *v_in, float *mu_out, float *m_out, float *v_out, float next_sigma,
                                  uint64_t next_gen, int64_t first_row, int32_t n_rows, int32_t per_rank, int32_t world,
                                  float *theta_next, float *best);
/* The same generation for R independent trials at once (csrc/ses_batch.hip) -- what a sweep driver that runs its trials one after
 * the other (sweep_main.py's trial loop around offspring_strategies.py:380-419) spends R x (3 or 4) latency-bound launches on.
 * Trial r owns rows [r n, (r + 1) n) of fitness and theta_next and row r of the [R, P] state matrices; everything it gets --
 * mu_out[r], m_out[r], v_out[r], its rows of theta_next, best[r] -- equals, bit for bit,
 *   ses_openai_generation(n, seed_r, gen_r, ..., next_sigma_r, next_gen_r, first_row 0, n_rows n) on that slice
 * (tests/test_gpu_batch.py): rank key, noise row and gradient chunks count from the trial's first row, row 0 of every trial is
 * its new mean.  The number of launches does not depend on R: counting rank, gradient, [update + population] for policies of up
 * to 1024 parameters; rank, gradient, update, population above.
 *   trials[R]: DEVICE memory written by the caller, one record per trial (the library copies nothing and does not synchronise);
 *   (mu, m, v)_in -> _out: distinct float32[R, P] buffers; theta_next[R n, P]; best: optional float32[R] <- max(fitness) per trial.
 * Limits: R >= 1, 2 <= n <= 8192 (the counting rank only; above: SES_ERR_UNSUPPORTED), R n <= 2^20.  Batch and solo calls may
 * alternate on one handle. */
typedef struct ses_batch_trial {
    uint64_t seed, gen, next_gen; /* Philox keys: the evaluated population's and the next one's */
    double   adam_a;              /* lr*sqrt(1-b2^t)/(1-b1^t), as for ses_openai_generation */
    float    update_factor;       /* (float)(-(lr / ((double)n * sigma))): the host expression of ses_openai_generation */
    float    next_sigma;
} ses_batch_trial;
int ses_openai_generation_batch(ses_handle *h, const float *fitness, int32_t R, int32_t n, const ses_batch_trial *trials,
                                const float *mu_in, const float *m_in, const float *v_in, float *mu_out, float *m_out,
                                float *v_out, float *theta_next, float *best);
/* The simple_evolution / simple_genetic generation for R independent trials at once (csrc/ses_batch_elite.hip).  The batch is
 * RAGGED: trial r owns rows [row0, row0 + n) of fitness and theta_next and the parent rows [parent0, parent0 + 1) (evolution: its
 * mu, parents_total = R) or [parent0, parent0 + elite_num) (genetic: its elites, best first, parents_total = sum of elite_num);
 * n and elite_num may differ between the trials.  Everything a trial gets -- its rows of parents_out and theta_next, alias_state[r],
 * best[r], its elite ids -- equals, bit for bit, what the solo sequence
 *   ses_rank_center -> ses_elite_select -> ses_perturb(row_ids, parent_idx) -> [ses_elite_mean] -> ses_perturb
 * gives for its slice alone (tests/test_gpu_batch_elite.py).  The parent maps are closed forms, no map array is passed:
 *   evolution  row 0 -> -1, row 1 -> -1, every other row -> 0   (population = [mu, mu, mu + noise ...])
 *   genetic    per = n / elite_num, e = i / per: row i -> -1 - e when i % per == 0, else e
 * An elite row is parents_in[..] verbatim for a negative entry, else fma(pop_sigma, z(seed, gen, id, quad), parents_in[..]); elite
 * rows are rebuilt from parents_in, never read from theta, so theta_next may be the buffer that held the evaluated population.
 * The next population is drawn from parents_out with next_sigma and next_gen, the noise row being the index within the trial.
 * Three launches whatever R: [rank + selection] one workgroup per trial, [parents], [population]; the last honours ses_set_stamp.
 *   trials[R]: DEVICE memory written by the caller (the library copies nothing and does not synchronise), so n_max = max n,
 *   k_max = max elite_num, rows_total and parents_total are host arguments; the kernels clamp every index derived from a record
 *   into [0, rows_total) / [0, parents_total): a table that disagrees with them gives wrong numbers, never a fault.
 *   parents_in -> parents_out: distinct float32[parents_total, P]; alias_state: int32[R], updated in place (evolution; NULL for
 *   genetic); best: optional float32[R], device or pinned; elite_ids_out: optional int32[parents_total] (genetic: trial r's ids at
 *   parent0) or int32[R * k_max] (evolution: at r * k_max).
 * Limits: R >= 1, 2 <= n <= 1024 per trial (above: SES_ERR_UNSUPPORTED), 1 <= elite_num <= n, rows_total <= 2^20.  May alternate
 * with solo calls and ses_openai_generation_batch on one handle. */
typedef struct ses_batch_elite_trial { /* 48 bytes */
    uint64_t seed, gen, next_gen;         /* Philox keys: the evaluated population's and the next one's */
    float    pop_sigma, next_sigma;       /* sigma the evaluated population was drawn with / the next one is drawn with */
    int32_t  row0, n, elite_num, parent0; /* first row and row count in fitness / theta_next; k; first row in parents_in / _out */
} ses_batch_elite_trial;
int ses_elite_generation_batch(ses_handle *h, int32_t strategy /* SES_STRATEGY_SIMPLE_EVOLUTION | _GENETIC */,
                               const float *fitness, int32_t R, const ses_batch_elite_trial *trials, int32_t n_max, int32_t k_max,
                               int32_t rows_total, int32_t parents_total, const float *parents_in, float *parents_out,
                               int32_t *alias_state, float *theta_next, float *best, int32_t *elite_ids_out);
/*
 * grad = (-lr / (n*sigma)) * sum_i weights[i] * eps_i ;  Adam (beta1 = 0.99, beta2 = 0.999, eps = 1e-8)
 * with step scale adam_a = lr*sqrt(1-beta2^t)/(1-beta1^t) computed by the host; mu, m, v updated in place.
 * _philox: eps_i regenerated from (seed, gen, row i) for ALL n rows -- every rank of a multi-GPU job
 *          computes the identical update without a second collective.  Row 0 has eps = 0
 *          (offspring_strategies.py:302-310) when skip_row0 != 0.
 * _stored: eps_store[n,P] from ses_perturb_host_noise, accumulated sequentially in the reference's
 *          order and precision (float32 accumulator, float64 products) -- bit-exact mirror.
 * grad_out (float32[P]) may be NULL.
 */
int ses_es_update_philox(ses_handle *h, const double *weights, int32_t n, int32_t skip_row0, uint64_t seed,
                         uint64_t gen, double lr, double sigma, double adam_a, float *mu, float *m, float *v,
                         float *grad_out);
int ses_es_update_stored(ses_handle *h, const double *weights, int32_t n, const float *eps_store, double lr,
                         double sigma, double adam_a, float *mu, float *m, float *v, float *grad_out);

/* ---- pgpe: PGPE with mirrored sampling and a per-parameter step size (csrc/ses_pgpe.hip; no reference counterpart) ---- */
/* The population of the pgpe strategy: n = 2 m rows in m pairs, no unperturbed row.  For pair j and parameter p, with z the
 * parameter-noise normal of (seed, gen, row = j, column = p) -- what ses_noise returns for row j --
 *   sig_p = fl(sigma * scale[p]);  d = fl(sig_p * z);  theta[2j][p] = fl(mu[p] + d);  theta[2j+1][p] = fl(mu[p] - d)
 * one rounding per operation, no fma.  mu, scale: float32[P]; theta[n_rows, P] receives the GLOBAL rows
 * [first_row, first_row + n_rows): any range gives the matching slice of the whole population, an odd first_row and a single
 * row included.  Stamps the tail time like ses_perturb (ses_set_stamp). */
int ses_perturb_mirrored(ses_handle *h, const float *mu, const float *scale, float sigma, uint64_t seed, uint64_t gen,
                         int64_t first_row, int32_t n_rows, float *theta);
/* One generation's tail of pgpe plus the next population, in the style of ses_openai_generation: counting rank (sort + search
 * above 8192 rows; the same kernels and tie rule), pair gradient, update, mirrored perturbation -- four launches (five); three (four)
 * where the update runs inside the perturbation launch ("pgpe_fused_apply_perturb").
 *   fitness[n]: the gathered fitness of the evaluated population (n even, >= 4; noise generation `gen`, drawn with `sigma` and
 *   scale_in).  With w_i the rank-centred weight of row i (the closed form of ses_rank_center, in double):
 *     d_j = (float)((w[2j] - w[2j+1]) / 2),  a_j = (float)((w[2j] + w[2j+1]) / 2)
 *     Gmu[p] = sum_j d_j z_jp,  Gs[p] = sum_j a_j fma(z_jp, z_jp, -1)
 *   float32 accumulators in an order that depends on n only: chunks of 1024 pairs, inside a chunk thread c of 256 takes the
 *   pairs c, c + 256, c + 512, c + 768 (fma chain), an 8-level tree adds the 256 threads (x[c] += x[c + s], s = 128 ... 1), the
 *   chunk partials are added in ascending order.  Then, with sig_p = fl((float)sigma * scale_in[p]) and m = n / 2:
 *     grad_mu = fl(fl(Gmu * sig_p) * (float)(-1 / m))  -> Adam as in ses_es_update_* (adam_a from the host), mu/m/v_in -> _out
 *     ds = fl(fl(Gs * scale_in) * (float)(sigma_learning_rate / m));  s1 = fl(scale_in + ds)
 *     s2 = min(max(s1, fl(scale_in * (float)(1 - sigma_max_change))), fl(scale_in * (float)(1 + sigma_max_change)))
 *     scale_out = min(max(s2, scale_lo), scale_hi)
 *   (mu, m, v, scale)_in -> _out: distinct float32[P] buffers, the caller ping-pongs them;
 *   theta_next[n_rows, P]: rows [first_row, first_row + n_rows) of the next population, drawn by ses_perturb_mirrored's kernel
 *   from (mu_out, scale_out, next_sigma, next_gen) (n_rows = 0: none; a sharded run calls this on every rank with the gathered
 *   fitness and its own rows: the replicated tail);  best: optional float32[1] <- max(fitness);
 *   gmu_out, gs_out: optional float32[P] <- Gmu, Gs. */
int ses_pgpe_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma, double adam_a,
                        double sigma_learning_rate, double sigma_max_change, float scale_lo, float scale_hi, const float *mu_in,
                        const float *m_in, const float *v_in, const float *scale_in, float *mu_out, float *m_out, float *v_out,
                        float *scale_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows,
                        float *theta_next, float *best, float *gmu_out, float *gs_out);

/* ---- ars: Augmented Random Search over the best mirrored directions (Mania, Guy & Recht 2018; csrc/ses_ars.hip; no reference
 * counterpart) ---- */
/* State: mu[P] (the zero network at the start); on the host curr_sigma (init_sigma, times sigma_decay after every evaluate;
 * sigma_decay = 1 is textbook ARS) and the generation key.  No Adam buffers, no scale vector.
 * Population: n = 2 m rows in m pairs (n even, >= 4), no unperturbed row.  With z the parameter-noise normal of (seed, gen, row = j,
 * column = p) -- what ses_noise returns for row j, no new stream tag --
 *   d = fl((float)sigma * z);  theta[2j][p] = fl(mu[p] + d);  theta[2j+1][p] = fl(mu[p] - d)
 * one rounding per operation, no fma: bit for bit ses_perturb_mirrored with scale = 1.0f everywhere (which is how a caller draws
 * the first population).  Rows are global: any [first_row, first_row + n_rows) gives the matching slice.
 * One generation's tail plus the next population.  fitness[n]: the gathered fitness of the evaluated population (noise generation
 * `gen`); b: the number of directions used, 1 <= b <= m.
 *   1. pair scores s_j = max(f[2j], f[2j+1]);
 *   2. the m scores are ranked by the kernels of every tail (counting rank up to 8192 entries, tile sort + search above), rule
 *      rank[j] = #{ i : s_i > s_j or (s_i == s_j and i > j) } -- a strict order: among equal scores the higher pair index comes
 *      first.  sel_k = the pair of rank k, k < b;
 *   3. sigma_R = the population standard deviation (divisor 2 b) of the 2 b values x_e = f[2 sel_{e / 2} + (e & 1)], e < 2 b, in
 *      DOUBLE, two passes: thread c of 256 adds x_c, x_{c + 256}, ... in ascending order to 0.0, an 8-level tree (x[c] += x[c + s],
 *      s = 128 ... 1) adds the threads; mean = sum / (2 b); the squared deviations fl(fl(x_e - mean)^2) are added the same way
 *      (product and sum rounded separately); sigma_R = sqrt(sum / (2 b)), correctly rounded.  The order depends on b only;
 *   4. d_k = (float)((double)f[2 sel_k] - (double)f[2 sel_k + 1]);
 *   5. G[p] = sum_k d_k z_{sel_k, p}, float32: chunks of 1024 SELECTED pairs in rank order, inside a chunk thread c of 256 takes
 *      k = c, c + 256, c + 512, c + 768 (fma chain from 0), the 8-level tree adds the 256 threads, the chunk partials are added in
 *      ascending order.  Unselected pairs draw no noise.  The order depends on (n, b) only;
 *   6. step = sigma_R > 0 ? (float)(learning_rate / ((double)b * sigma_R)) : 0.0f  (formed on the device);
 *   7. mu_out[p] = fl(mu_in[p] + fl(step * G[p])).  With all selected returns equal sigma_R = 0 and mu_out = mu_in bit for bit;
 *   8. best = the score of the pair of rank 0 = max(fitness).
 * `sigma` (what the evaluated population was drawn with) does not enter the update: the division by sigma_R takes its place.
 * mu_in -> mu_out: distinct float32[P] buffers; theta_next[n_rows, P]: rows [first_row, first_row + n_rows) of the next population
 * from (mu_out, next_sigma, next_gen) (n_rows = 0: none; a sharded run calls this on every rank with the gathered fitness and its own
 * rows: the replicated tail);  best: optional float32[1];  g_out: optional float32[P] <- G;  sigma_r_out: optional double[1] <-
 * sigma_R.  Launches: scores, rank (two above 8192 pairs), gradient + sigma_R, update + perturbation -- four; five where the update is
 * a launch of its own (more than 1024 parameters, more than 16 chunks, n_rows = 0, or "ars_fused_apply_perturb" = 0).  A fitness
 * vector with NaNs has no strict order; the result is then unspecified, but every access stays inside the population. */
int ses_ars_generation(ses_handle *h, const float *fitness, int32_t n, int32_t b, uint64_t seed, uint64_t gen, double sigma,
                       double learning_rate, const float *mu_in, float *mu_out, float next_sigma, uint64_t next_gen,
                       int64_t first_row, int32_t n_rows, float *theta_next, float *best, float *g_out, double *sigma_r_out);
/* The same generation for R independent trials at once (csrc/ses_batch_ars.hip) -- what a sweep that runs its ars trials one after
 * the other spends R x 4 latency-bound launches on.  Trial r owns rows [r n, (r + 1) n) of fitness and theta_next (a fixed stride:
 * the trials share offspring_num), with m = n / 2 the pairs [r m, (r + 1) m), and row r of mu_in / mu_out float32[R, P], best[R],
 * g_out[R, P] and sigma_r_out[R]; everything it gets -- mu_out[r], its n rows of theta_next, best[r], g_out[r], sigma_r_out[r] --
 * equals, bit for bit,
 *   ses_ars_generation(n, b_r, seed_r, gen_r, ., learning_rate_r, ..., next_sigma_r, next_gen_r, first_row 0, n_rows n) on that slice
 * (tests/test_gpu_batch_ars.py).  The orders are ses_ars_generation's (steps 1 - 8 above), pairs and rows counted from the trial's
 * first: pair j of trial r draws (seed_r, gen_r, row j); the counting rank of the m scores with key (ordered bits, index within the
 * trial), -0 as +0; sigma_R in double, thread c of 256 taking the elements c, c + 256, ... ascending from 0.0, the 8-level tree,
 * product and sum rounded separately, the root correctly rounded; the step formed on the device from learning_rate_r, b_r and
 * sigma_R; G in chunks of 1024 SELECTED pairs in rank order, thread c taking k = c, c + 256, c + 512, c + 768 (an fma chain from
 * 0), the 8-level tree, then exactly the trial's own ceil(b_r / 1024) chunk partials in ascending order -- no zero partial of a
 * chunk the trial does not have is added (+0.0 would turn a -0 sum into +0); mu' = fl(mu + fl(step * G)); the population with
 * d = fl(next_sigma * z), mu' +- d, no fma.  Only the selection is ragged: b_r = elite_num_r sets the length of a trial's selected
 * list and the number of its chunks.  Four launches whatever R (scores, rank, gradient + sigma_R, update + population), five where
 * the solo call takes five (more than 1024 parameters, or "ars_fused_apply_perturb" = 0); the trial is a grid dimension of each and
 * no workgroup waits for another.  The table is DEVICE memory the caller wrote (the library copies nothing and does not
 * synchronise):
 *   trials[R]: one ses_batch_ars_trial per trial and generation -- everything in it is a function of the generation number;
 *   b[R]: HOST memory, the trials' b_r, read for the checks below and for sizing the grid (ceil(max b / 1024) chunks); the kernels
 *     read trials[r].b and clamp it into [1, m], hold a trial to the chunks the grid has, and clamp every entry read from a selected
 *     list into the trial's own m pairs: a table that disagrees with b[], or a fitness vector with NaNs, gives wrong numbers, never
 *     an access outside the trial's slice;
 *   mu_in -> mu_out: distinct buffers; theta_next[R n, P]; best: optional float32[R], device or pinned; g_out: optional
 *   float32[R, P] <- G; sigma_r_out: optional double[R] <- sigma_R.
 * The population launch honours ses_set_stamp and leaves the R m rank entries zeroed, like the solo call's.
 * Limits: R >= 1, n even, 4 <= n <= 16384 (m <= 8192, the counting rank only; above: SES_ERR_UNSUPPORTED), R n <= 2^20,
 * 1 <= b_r <= m.  May alternate with solo calls and with the other three batch calls on one handle. */
typedef struct ses_batch_ars_trial { /* 40 bytes */
    uint64_t seed, gen, next_gen; /* Philox keys: the evaluated population's and the next one's */
    double   learning_rate;
    float    next_sigma;          /* (float) of the sigma the next population is drawn with */
    int32_t  b;                   /* the directions used, 1 <= b <= n / 2 */
} ses_batch_ars_trial;
int ses_ars_generation_batch(ses_handle *h, const float *fitness, int32_t R, int32_t n, const int32_t *b,
                             const ses_batch_ars_trial *trials, const float *mu_in, float *mu_out, float *theta_next, float *best,
                             float *g_out, double *sigma_r_out);

/* ---- sep_cma_es: diagonal CMA-ES (Ros & Hansen 2008) with a step size adapted on the device (csrc/ses_sepcma.hip; no reference
 * counterpart) ---- */
/* The constants of the strategy, formed once by the host in double from (n, P, mu) -- mu = the number of selected rows, default
 * n / 2 -- with w_k proportional to ln(mu + 0.5) - ln(k + 1), k < mu, normalised to sum 1 (the float32 table weights[mu]):
 *   mueff = 1 / sum w^2;  c_sigma = (mueff + 2) / (P + mueff + 5);  d_sigma = 1 + 2 max(0, sqrt((mueff - 1) / (P + 1)) - 1) + c_sigma
 *   c_c = (4 + mueff / P) / (P + 4 + 2 mueff / P);  c_1 = min(1, (P + 2) / 3 * 2 / ((P + 1.3)^2 + mueff))
 *   c_mu = min(1 - c_1, (P + 2) / 3 * 2 (mueff - 2 + 1 / mueff) / ((P + 2)^2 + mueff));  chi = sqrt(P) (1 - 1 / (4 P) + 1 / (21 P^2))
 * scale_lo / scale_hi bound sqrt(C[p]) (C is clamped to [fl(scale_lo * scale_lo), fl(scale_hi * scale_hi)], float32 products),
 * step_lo / step_hi bound the step factor. */
typedef struct ses_sepcma_params {
    int32_t mu, reserved;
    double mueff, c_sigma, d_sigma, c_c, c_1, c_mu, chi;
    float scale_lo, scale_hi, step_lo, step_hi;
} ses_sepcma_params;
/* The population of sep_cma_es: n rows, no unperturbed row, no mirroring.  With z the parameter-noise normal of (seed, gen, row
 * = i, column = p) -- what ses_noise returns for row i --
 *   theta[i][p] = fl(mu[p] + fl(fl(fl(sigma * step[0]) * sqrt(C[p])) * z))
 * one rounding per operation, no fma, sqrt correctly rounded.  mu, C: float32[P]; step: float32[1] ON THE DEVICE; theta[n_rows, P]
 * receives the GLOBAL rows [first_row, first_row + n_rows).  Stamps the tail time like ses_perturb (ses_set_stamp). */
int ses_perturb_sepcma(ses_handle *h, const float *mu, const float *C, const float *step, float sigma, uint64_t seed, uint64_t gen,
                       int64_t first_row, int32_t n_rows, float *theta);
/* One generation's tail of sep_cma_es plus the next population, in the style of ses_pgpe_generation: counting rank (sort + search
 * above 8192 rows; the same kernels and tie rule), weighted sums, update, perturbation -- four launches (five).
 *   fitness[n]: the gathered fitness of the evaluated population (n >= 4; noise generation `gen`, drawn with `sigma` and
 *   (C, step)_in).  With w_i = weights[rank_i] if rank_i < p->mu, else 0:
 *     Sz[p] = sum_i w_i z_ip,  Szz[p] = sum_i w_i fl(z_ip z_ip)
 *   float32 accumulators in an order that depends on n only: chunks of 1024 rows, inside a chunk thread c of 256 takes the rows
 *   c, c + 256, c + 512, c + 768 (an fma chain; rows with rank >= mu are skipped and draw nothing), an 8-level tree adds the 256
 *   threads (x[c] += x[c + s], s = 128 ... 1), the chunk partials are added in ascending order.  Then ONE workgroup of 1024 threads:
 *     p_sigma' = fl(fl(a_s p_sigma) + fl(b_s Sz)),  a_s = (float)(1 - c_sigma),  b_s = (float)sqrt(c_sigma (2 - c_sigma) mueff)
 *     norm2 = sum_p (double)p_sigma'[p]^2 in double: thread c adds the squares of p = c, c + 1024, ... in ascending order to 0.0,
 *             a 10-level tree adds the 1024 threads (x[c] += x[c + s], s = 512 ... 1)
 *     one thread, in double:  nrm = sqrt(norm2);  h = nrm * hsig_scale < (1.4 + 2 / (P + 1)) * chi
 *             step' = min(max((float)((double)step * exp(min(1, (c_sigma / d_sigma) * (nrm / chi - 1)))), step_lo), step_hi)
 *             (hsig_scale = 1 / sqrt(1 - (1 - c_sigma)^(2 t)) comes from the host, t = the number of this update, from 1)
 *     s = sqrt(C);  y = fl(s Sz);  p_c' = fl(fl(a_c p_c) + fl(hb y)),  a_c = (float)(1 - c_c),  hb = h ? (float)sqrt(c_c (2 - c_c) mueff) : 0
 *     mu' = fl(mu + fl(fl(fl((float)sigma * step) * s) * Sz))        (the deviation the evaluated population was drawn with)
 *     C' = min(max(fl(fl(fl(k0 C) + fl(c1f fl(p_c' p_c'))) + fl(cmuf fl(C Szz))), fl(scale_lo scale_lo)), fl(scale_hi scale_hi))
 *             k0 = (float)(1 - c_1 - c_mu + (h ? 0 : c_1 c_c (2 - c_c))),  c1f = (float)c_1,  cmuf = (float)c_mu
 *             (min / max are fminf / fmaxf, for C' and for step' alike: a NaN operand -- possible only with a NaN in the state
 *             or sums that overflowed, never with finite inputs inside the limits -- comes out as the LOWER limit, where a
 *             NaN-propagating min / max such as numpy's would return NaN)
 *   (mu, C, p_sigma, p_c, step)_in -> _out: distinct buffers (float32[P]; step float32[1]), the caller ping-pongs them;
 *   theta_next[n_rows, P]: rows [first_row, first_row + n_rows) of the next population, drawn by ses_perturb_sepcma's kernel from
 *   (mu_out, C_out, step_out, next_sigma, next_gen) (n_rows = 0: none; a sharded run calls this on every rank with the gathered
 *   fitness and its own rows: the replicated tail);  best: optional float32[1] <- max(fitness);
 *   sz_out, szz_out: optional float32[P] <- Sz, Szz;  norm2_out: optional double[1] <- norm2. */
int ses_sepcma_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma, double hsig_scale,
                          const ses_sepcma_params *p, const float *weights, const float *mu_in, const float *C_in,
                          const float *ps_in, const float *pc_in, const float *step_in, float *mu_out, float *C_out, float *ps_out,
                          float *pc_out, float *step_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows,
                          float *theta_next, float *best, float *sz_out, float *szz_out, double *norm2_out);
/* The same generation for R independent trials at once (csrc/ses_batch_sepcma.hip) -- what a sweep that runs its sep_cma_es trials
 * one after the other spends R x 4 latency-bound launches on.  Trial r owns rows [r n, (r + 1) n) of fitness and theta_next (a
 * fixed stride: the trials share offspring_num) and row r of the state matrices mu, C, ps, pc float32[R, P] and step float32[R];
 * everything it gets -- its rows of (mu, C, ps, pc, step)_out and of theta_next, best[r] -- equals, bit for bit,
 *   ses_sepcma_generation(n, seed_r, gen_r, sigma_r, hsig_scale_r, params_r, weights_r, ..., next_sigma_r, next_gen_r, first_row 0,
 *                         n_rows n) on that slice
 * (tests/test_gpu_batch_sepcma.py).  The orders are ses_sepcma_generation's, rows counted from the trial's first row: the counting
 * rank with key (ordered fitness bits, index within the trial), -0 as +0; Sz / Szz in chunks of 1024 rows, thread c of 256 taking
 * rows c, c + 256, c + 512, c + 768 (an fma chain, rows of rank >= mu_r skipped), the 8-level tree, the chunk partials in ascending
 * order; the update in ONE workgroup of 1024 threads PER TRIAL, norm2 in double with the 10-level tree, the scalar path in double on
 * one thread; the perturbation with s0 = fl(sigma * step_out[r]), no fma.  Only the selection is ragged: mu_r and with it the
 * weights and every constant may differ between the trials.  Four launches whatever R (rank, sums, update, population), the trial
 * a grid dimension of each; no workgroup waits for another.  The tables are DEVICE memory the caller wrote (the library copies
 * nothing and does not synchronise):
 *   trials[R]: one ses_batch_sepcma_trial per trial and generation -- everything in it is a function of the generation number;
 *   consts[R]: one ses_batch_sepcma_consts per trial, fixed over the run: from ses_sepcma_params and P by the host expressions of
 *     ses_sepcma_generation, in double, cast once --
 *       a_s = (float)(1 - c_sigma)   b_s = (float)sqrt(c_sigma (2 - c_sigma) mueff)   a_c = (float)(1 - c_c)
 *       hb1 = (float)sqrt(c_c (2 - c_c) mueff)   c1f = (float)c_1   cmuf = (float)c_mu   k0_h1 = (float)(1 - c_1 - c_mu + 0.0)
 *       k0_h0 = (float)(1 - c_1 - c_mu + c_1 c_c (2 - c_c))   var_lo = fl(scale_lo scale_lo)   var_hi = fl(scale_hi scale_hi)
 *       hsig_thr = (1.4 + 2 / (P + 1)) chi   cs_over_ds = c_sigma / d_sigma
 *   weights: float32[R, n], row r = trial r's mu_r weights, then zeros;
 *   mu[R]: HOST memory, the trials' mu_r, read for the checks below only; the kernels read consts[r].mu and clamp it into [1, n],
 *     so a table that disagrees gives wrong numbers, never an access outside the caller's buffers;
 *   (mu, C, ps, pc, step)_in -> _out: distinct buffers; theta_next[R n, P]; best: optional float32[R], device or pinned.
 * The population launch honours ses_set_stamp and leaves the rank vector zeroed, like the solo call's.
 * Limits: R >= 1, 4 <= n <= 8192 (the counting rank only; above: SES_ERR_UNSUPPORTED), R n <= 2^20, 1 <= mu_r <= n.  May alternate
 * with solo calls, ses_openai_generation_batch and ses_elite_generation_batch on one handle. */
typedef struct ses_batch_sepcma_trial { /* 40 bytes */
    uint64_t seed, gen, next_gen; /* Philox keys: the evaluated population's and the next one's */
    double   hsig_scale;          /* 1 / sqrt(1 - (1 - c_sigma)^(2 t)), t = the number of this update, from 1 */
    float    sigma, next_sigma;   /* (float) of the sigma the evaluated population was drawn with / the next one is drawn with */
} ses_batch_sepcma_trial;
typedef struct ses_batch_sepcma_consts { /* 80 bytes */
    double  hsig_thr, cs_over_ds, chi;
    float   a_s, b_s, a_c, hb1, c1f, cmuf, k0_h1, k0_h0, var_lo, var_hi, step_lo, step_hi;
    int32_t mu, reserved;
} ses_batch_sepcma_consts;
int ses_sepcma_generation_batch(ses_handle *h, const float *fitness, int32_t R, int32_t n, const int32_t *mu,
                                const ses_batch_sepcma_trial *trials, const ses_batch_sepcma_consts *consts, const float *weights,
                                const float *mu_in, const float *C_in, const float *ps_in, const float *pc_in, const float *step_in,
                                float *mu_out, float *C_out, float *ps_out, float *pc_out, float *step_out, float *theta_next,
                                float *best);

/* ---- lm_ma_es: limited-memory matrix adaptation ES (Loshchilov, Glasmachers & Beyer 2019) with a step size adapted on the device
 * (csrc/ses_lmma.hip; no reference counterpart) ---- */
/* The constants of the strategy, formed once by the host in double from (n, P, mu, m): mu, the weight table w_k (float32
 * weights[mu]), mueff, c_sigma, d_sigma and chi exactly as for sep_cma_es (ses_sepcma_params); m = the number of direction vectors
 * ("memory", 0 .. SES_LMMA_MAX_MEMORY; 0 = isotropic ES with cumulative step-size adaptation); and for j < m
 *   c_d[j] = 1 / (1.5^j P),  c_c[j] = min(1, n / (4^j P))
 *   cd[j] = (float)c_d[j],  ad[j] = (float)(1 - c_d[j]),  ac[j] = (float)(1 - c_c[j]),  bc[j] = (float)sqrt(mueff c_c[j] (2 - c_c[j]))
 * (entries from m on are not read).  step_lo / step_hi bound the step factor.  The kernels hold at most SES_LMMA_MAX_P parameters
 * per row; a handle with more gets SES_ERR_UNSUPPORTED from both entry points. */
#define SES_LMMA_MAX_MEMORY 32
#define SES_LMMA_MAX_P 16384
typedef struct ses_lmma_params {
    int32_t mu, m;
    double mueff, c_sigma, d_sigma, chi;
    float step_lo, step_hi;
    float cd[SES_LMMA_MAX_MEMORY], ad[SES_LMMA_MAX_MEMORY], ac[SES_LMMA_MAX_MEMORY], bc[SES_LMMA_MAX_MEMORY];
} ses_lmma_params;
/* The population of lm_ma_es: n rows, no unperturbed row, no mirroring.  M: float32[m, P] row-major, the direction vectors, of
 * which the first m_active (0 <= m_active <= p->m) are used.  With z_i the parameter-noise normals of (seed, gen, row = i) -- what
 * ses_noise returns for row i --
 *   v_0 = z_i;  for j = 0 .. m_active - 1:
 *     dot_j = sum_p M[j][p] v_j[p]                       (float32, fma; the order below)
 *     g_j = fl(cd[j] dot_j)
 *     v_{j+1}[p] = fl(fl(ad[j] v_j[p]) + fl(g_j M[j][p]))
 *   theta[i][p] = fl(mu[p] + fl(fl(sigma * step[0]) * v_last[p]))
 * one rounding per operation and no fma outside the dots.  Order of dot_j (it depends on P only): the row is held by T threads,
 * T = 64 for P <= 256 and 256 above; thread c owns the quads q = c, c + T, ... (parameters 4q .. 4q + 3).  (1) four fma chains
 * per thread, one per position l = 0..3 inside a quad, each over the thread's quads in ascending order from +0:
 * a_l = fma(M[j][4q + l], v_j[4q + l], a_l);  (2) x = (a_0 + a_1) + (a_2 + a_3);  (3) over the 64 lanes of a wave (thread c =
 * lane c % 64 of wave c / 64) x[lane] = x[lane] + x[lane ^ s] for s = 32, 16, 8, 4, 2, 1;  (4) T = 256: with w[0..3] the four wave
 * sums, (w[0] + w[2]) + (w[1] + w[3]).
 * mu: float32[P]; step: float32[1] ON THE DEVICE; theta[n_rows, P] receives the GLOBAL rows [first_row, first_row + n_rows);
 * dots_out: optional float32[n_rows, m_active] <- dot_j of each row.  Stamps the tail time like ses_perturb (ses_set_stamp). */
int ses_perturb_lmma(ses_handle *h, const float *mu, const float *M, const float *step, const ses_lmma_params *p, int32_t m_active,
                     float sigma, uint64_t seed, uint64_t gen, int64_t first_row, int32_t n_rows, float *theta, float *dots_out);
/* One generation's tail of lm_ma_es plus the next population, in the style of ses_sepcma_generation: counting rank (sort + search
 * above 8192 rows; the same kernels and tie rule), weighted sums, update, perturbation -- four launches (five).
 *   fitness[n]: the gathered fitness of the evaluated population (n >= 4; noise generation `gen`, drawn with `sigma`, (M, step)_in
 *   and m_active vectors).  With w_i = weights[rank_i] if rank_i < p->mu, else 0:
 *     Sz[p] = sum_i w_i z_ip      in ses_sepcma_generation's order (its sums kernel, launched as it is; Szz is formed and not read)
 *   Then ONE workgroup of 1024 threads:
 *     p_sigma' = fl(fl(a_s p_sigma) + fl(b_s Sz)),  a_s = (float)(1 - c_sigma),  b_s = (float)sqrt(c_sigma (2 - c_sigma) mueff)
 *     norm2 = sum_p (double)p_sigma'[p]^2 in double, in ses_sepcma_generation's order
 *     one thread, in double:  step' = min(max((float)((double)step * exp(min(1, (c_sigma / d_sigma) * (sqrt(norm2) / chi - 1)))),
 *             step_lo), step_hi)        (fminf / fmaxf: a NaN comes out as the LOWER limit, as for sep_cma_es; there is no h term)
 *     u_0 = Sz;  for j = 0 .. m_active - 1, with the OLD vectors:
 *       sdot_j = sum_p M[j][p] u_j[p]: thread c takes p = c, c + 1024, ... in ascending order as ONE fma chain from +0; over the 64
 *             lanes of a wave x[lane] = x[lane] + x[lane ^ s], s = 32 ... 1; with w[0..15] the sixteen wave sums, y[k] = w[k] and
 *             y[k] = y[k] + y[k ^ s] for s = 8, 4, 2, 1
 *       u_{j+1}[p] = fl(fl(ad[j] u_j[p]) + fl(fl(cd[j] sdot_j) M[j][p]))
 *     mu' = fl(mu + fl(fl((float)sigma * step) * u_last))          (the old step; in exact arithmetic u_last = sum_i w_i v_i)
 *     M'[j][p] = fl(fl(ac[j] M[j][p]) + fl(bc[j] Sz[p]))           for every j < p->m
 *   (mu, p_sigma, M, step)_in -> _out: distinct buffers (float32[P], float32[m, P]; step float32[1]), the caller ping-pongs them
 *   (M may be NULL when m = 0);  theta_next[n_rows, P]: rows [first_row, first_row + n_rows) of the next population, drawn by
 *   ses_perturb_lmma's kernel from (mu_out, M_out, step_out, m_active_next, next_sigma, next_gen) (n_rows = 0: none; a sharded run
 *   calls this on every rank with the gathered fitness and its own rows: the replicated tail);  best: optional float32[1] <-
 *   max(fitness);  sz_out, sd_out: optional float32[P] <- Sz, u_last;  sdots_out: optional float32[m_active] <- sdot_j;  norm2_out:
 *   optional double[1] <- norm2;  dots_next_out: optional float32[n_rows, m_active_next] <- the dots of the next population's rows. */
int ses_lmma_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma,
                        const ses_lmma_params *p, const float *weights, int32_t m_active, int32_t m_active_next, const float *mu_in,
                        const float *ps_in, const float *M_in, const float *step_in, float *mu_out, float *ps_out, float *M_out,
                        float *step_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows, float *theta_next,
                        float *best, float *sz_out, float *sd_out, float *sdots_out, double *norm2_out, float *dots_next_out);

/* ---- ma_es: matrix adaptation ES with the full transformation matrix (Beyer & Sendhoff 2017) and a step size adapted on the device
 * (csrc/ses_maes.hip; no reference counterpart).  For policies of up to SES_MAES_MAX_P parameters: a handle with more gets
 * SES_ERR_UNSUPPORTED from both entry points (lm_ma_es serves those). ---- */
/* The constants of the strategy, formed once by the host in double from (n, P, mu): mu, the weight table w_k (float32 weights[mu]),
 * mueff, c_sigma, d_sigma and chi exactly as for sep_cma_es (ses_sepcma_params); the full-matrix rates
 *   c_1 = 2 / ((P + 1.3)^2 + mueff),  c_mu = min(1 - c_1, 2 (mueff - 2 + 1 / mueff) / ((P + 2)^2 + mueff))
 * and what the update multiplies with:  a_m = (float)(1 - c_1 / 2 - c_mu / 2),  c1h = (float)(c_1 / 2),  cmuh = (float)(c_mu / 2).
 * step_lo / step_hi bound the step factor. */
#define SES_MAES_MAX_P 1024
typedef struct ses_maes_params {
    int32_t mu, reserved;
    double mueff, c_sigma, d_sigma, chi, c_1, c_mu;
    float a_m, c1h, cmuh, step_lo, step_hi;
} ses_maes_params;
/* The population of ma_es: n rows, no unperturbed row, no mirroring.  M: float32[P, P] row-major.  With z_i the parameter-noise
 * normals of (seed, gen, row = i) -- what ses_noise returns for row i --
 *   D[i][p] = sum_q M[p][q] z_i[q]:  ONE chain acc = fma(z_i[q], M[p][q], acc) from +0 over q = 0, 1, ..., P - 1; an odd P adds
 *             fma(+0, +0, acc) once more (the GEMM D = Z M^T on v_mfma_f32_32x32x2_f32, one accumulator per 32 x 32 tile, k-blocks
 *             ascending: the instruction adds its two products one after the other with one rounding each)
 *   theta[i][p] = fl(mu[p] + fl(fl(sigma * step[0]) * D[i][p]))
 * The order depends on P only: any row range gives the bits of the whole population's rows.  mu: float32[P]; step: float32[1] ON
 * THE DEVICE; theta[n_rows, P] and d_out[n_rows, P] receive the GLOBAL rows [first_row, first_row + n_rows); either may be NULL, not
 * both.  Z is never stored.  Stamps the tail time like ses_perturb (ses_set_stamp). */
int ses_perturb_maes(ses_handle *h, const float *mu, const float *M, const float *step, float sigma, uint64_t seed, uint64_t gen,
                     int64_t first_row, int32_t n_rows, float *theta, float *d_out);
/* One generation's tail of ma_es plus the next population, in the style of ses_lmma_generation: counting rank (sort + search above
 * 8192 rows; the same kernels and tie rule), weighted sums, vectors, matrix-vector products, matrix update, perturbation -- six
 * launches (seven; one more where d_in is NULL).
 *   fitness[n]: the gathered fitness of the evaluated population (n >= 4; noise generation `gen`, drawn with `sigma` and
 *   (M, step)_in); d_in: float32[n, P], the D of ALL n rows as ses_perturb_maes wrote it, or NULL: the call then recomputes it
 *   with that kernel (the same bits: this is how the replicated tail of a sharded run gets rows it never drew).
 *   With w_i = weights[rank_i] if rank_i < p->mu, else 0:
 *     Sz[p] = sum_i w_i z_ip      in ses_sepcma_generation's order (its sums kernel, launched as it is; Szz is formed and not read)
 *     p_sigma' = fl(fl(a_s p_sigma) + fl(b_s Sz)),  a_s = (float)(1 - c_sigma),  b_s = (float)sqrt(c_sigma (2 - c_sigma) mueff)
 *     norm2 = sum_p (double)p_sigma'[p]^2 in double, in ses_sepcma_generation's order
 *     one thread, in double:  step' = min(max((float)((double)step * exp(min(1, (c_sigma / d_sigma) * (sqrt(norm2) / chi - 1)))),
 *             step_lo), step_hi)        (fminf / fmaxf: a NaN comes out as the LOWER limit, as for sep_cma_es; there is no h term)
 *     Sd[p] = sum_q M[p][q] Sz[q],  qv[p] = sum_q M[p][q] p_sigma'[q]  with the OLD M, each in this order (it depends on P only):
 *             64 chains, chain l over q = l, l + 64, l + 128, ... ascending, acc = fma(M[p][q], x[q], acc) from +0; then
 *             y[l] = y[l] + y[l ^ s] for s = 32, 16, 8, 4, 2, 1 (a butterfly: every l ends with the same bits)
 *     mu' = fl(mu + fl(fl((float)sigma * step) * Sd))             (the old step; in exact arithmetic Sd = sum_i w_i D_i)
 *     G[p][q] = sum over the selected rows (rank_i < mu) of fl(w_i D[i][p]) z_i[q]:  ONE chain acc = fma(fl(w_i D[i][p]), z_i[q], acc)
 *             from +0 over the selected rows in ascending ROW index i; an odd count adds fma(+0, +0, acc) once more (the GEMM
 *             (W D)^T Z on the same instruction, one accumulator per 32 x 32 tile)
 *     M'[p][q] = fl(fl(fl(a_m M[p][q]) + fl(c1h fl(qv[p] p_sigma'[q]))) + fl(cmuh G[p][q]))
 *   which is M (a I + c_1 / 2 p p^T + c_mu / 2 sum w z z^T) with M multiplied through: M z_i is the D_i the population was drawn
 *   with, so the update costs P^2 mu, not P^3.
 *   (mu, p_sigma, M, step)_in -> _out: distinct buffers (float32[P], float32[P], float32[P, P], float32[1]), the caller ping-pongs
 *   them;  theta_next[n_rows, P], d_next_out[n_rows, P] (optional): rows [first_row, first_row + n_rows) of the next population and of
 *   its D, by ses_perturb_maes's kernel from (mu_out, M_out, step_out, next_sigma, next_gen) (n_rows = 0: none; a sharded run calls
 *   this on every rank with the gathered fitness, d_in = NULL and its own rows: the replicated tail);  d_next_out must not be d_in;
 *   best: optional float32[1] <- max(fitness);  sz_out, sd_out, qv_out: optional float32[P] <- Sz, Sd, qv;  g_out: optional
 *   float32[P, P] <- G;  norm2_out: optional double[1] <- norm2. */
int ses_maes_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma,
                        const ses_maes_params *p, const float *weights, const float *mu_in, const float *ps_in, const float *M_in,
                        const float *step_in, const float *d_in, float *mu_out, float *ps_out, float *M_out, float *step_out,
                        float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows, float *theta_next, float *d_next_out,
                        float *best, float *sz_out, float *sd_out, float *qv_out, float *g_out, double *norm2_out);

/* ---- K6: elite selection + mean (offspring_strategies.py:112-116, 234-248) ------------------ */
/* elite_ids[j] = index of the offspring with rank j, j < k. */
int ses_elite_ids(ses_handle *h, const int32_t *rank, int32_t n, int32_t k, int32_t *elite_ids);
/* The elite bookkeeping of one generation in a single launch, nothing read back by the host:
 *   elite_ids[j]        = index of the offspring with rank j (as ses_elite_ids);
 *   elite_parent_idx[j] = parent_map[elite_ids[j]], the entry of the current population's parent map -- what
 *                         ses_perturb(row_ids = elite_ids, parent_idx = elite_parent_idx) needs to rebuild the rows;
 *   alias_first[j]      = the flags of ses_elite_mean for simple_evolution (offspring_strategies.py:234-248 sums the
 *                         elites into elite 0 in place; while population slots 0 and 1 are the same module object,
 *                         an elite in the other of the two slots doubles the running sum): set when *alias_state != 0,
 *                         elite_ids[0] is 0 or 1, and elite_ids[j] is the other of 0 / 1;
 *   *alias_state        is then updated: elite_ids[0] == 0, or elite_ids[0] == 1 while the state was set.
 * alias_state and alias_first may be NULL together (simple_genetic).  k <= 1024. */
int ses_elite_select(ses_handle *h, const int32_t *rank, int32_t n, int32_t k, const int32_t *parent_map,
                     int32_t *alias_state, int32_t *elite_ids, int32_t *elite_parent_idx, int32_t *alias_first);
/* rows[k,P] (the elites, best first) -> mean[P] = ((rows[0] + rows[1]) + ... ) / k in float32, the
 * reference's in-place order (:241-248).  alias_first[j] != 0 (j >= 1) marks an elite that is the same
 * module object as elite 0, for which the reference's `mu += elite` doubles the running sum
 * (SURVEY 3.4-6); NULL = no aliasing. */
int ses_elite_mean(ses_handle *h, const float *rows, const int32_t *alias_first, int32_t k, float *mean);
/* dst[i,:] = src[ids[i],:] */
int ses_gather_rows(ses_handle *h, const float *src, const int32_t *ids, int32_t n_ids, float *dst);

/* ---- k whole generations per call (learning_strategies/evolution/loop.py:61-104 from C) ------------------------------------ */
/*
 * The generation loop of ESLoop.run() -- env resets, fused rollout, episode mean, strategy.evaluate, next population -- for
 * k generations in ONE call: the same entry points as above issued back to back from C, with the strategies' host-side
 * scalars (sigma decay, Adam's step scale, generation keys) advanced exactly as the Python classes advance them, so the
 * results are bit-identical to k per-generation calls.  Why: a generation of the reference's own configs (96-240
 * offspring) is 60-120 us of kernels and took ~96 us of Python to enqueue; from C the device is the limit.
 * Counter-based noise only.  Everything is enqueued, nothing is waited for.
 * Sharded runs (world > 1, one process per GPU): the rollout covers this rank's n_local rows, ses_allgather_fitness on `comm`
 * (the handle that owns the transports; same device and stream) gathers the shards inside the loop, openai_es continues
 * with ses_openai_generation_sharded where ses_openai_sharded_ok allows it, everything else with the replicated tail over
 * all n rows.  A peer-store time-out is the caller's to poll (ses_comm_p2p_status) at its own boundaries.
 *
 * ses_gen_state: the caller fills the fixed part and the buffers once, the call advances the rest in place:
 *   strategy            SES_STRATEGY_*
 *   n                   population rows: openai_es offspring_num (row 0 = mu); simple_evolution offspring_num + 1
 *                       ([mu, elite0, children]); simple_genetic elite_num * (offspring_num / elite_num)
 *   theta[2], parents[2], adam_m[2], adam_v[2]   ping-pong halves, `cur` says which holds the current generation's;
 *                       parents: mu[P] (openai_es, simple_evolution) or elites[elite_num, P] (simple_genetic)
 *   parent_map          int32[n] on the device, the strategy's constant map as for ses_perturb (elite strategies)
 *   alias_state         int32[1] on the device (simple_evolution, see ses_elite_select)
 *   fitness[n] (sharded: [world * per_rank], the gathered vector), init[(shared_init ? 1 : rows of theta) * E * init_width],
 *   work_i32[n + 3 * elite_num], work_f32[elite_num * P]
 *   world, first_row, n_local, per_rank, comm, fit_local   sharded runs only (world <= 1: ignored): this rank owns the global
 *                       rows [first_row, first_row + n_local) with first_row = rank * per_rank, per_rank = ceil(n / world);
 *                       theta[] then has n_local rows; fit_local[per_rank] receives this rank's fitness, its tail
 *                       [n_local, per_rank) holds -inf, written once by the caller
 *   sigma / pop_sigma   curr_sigma of the strategy / the sigma the current population was drawn with
 *   pop_gen             generation key of the current population (its noise and its env resets)
 *   adam_t              Adam's step counter
 *   scale[2], sigma_learning_rate, sigma_max_change, scale_lo, scale_hi   SES_STRATEGY_PGPE only (at the END of the struct: callers
 *                       that fill it by field name are unaffected): the per-parameter step sizes, ping-pong halves like parents[],
 *                       and the scalars of ses_pgpe_generation.  n = offspring_num (even, >= 4; no mu row), parents = mu[P], the
 *                       Adam buffers as for openai_es.  One GPU only: world > 1 with this strategy is SES_ERR_UNSUPPORTED
 *                       (sharded runs call ses_pgpe_generation per generation).
 *   cma_C[2], cma_ps[2], cma_pc[2], cma_step[2], cma_weights, cma   SES_STRATEGY_SEP_CMA_ES only (appended after the pgpe fields): the
 *                       variances, the two evolution paths and the step factor (float32[1]) as ping-pong halves like parents[], the
 *                       float32 weight table [cma.mu] and the constants of ses_sepcma_generation.  n = offspring_num (>= 4; no mu
 *                       row), parents = mu[P]; adam_t counts the updates (hsig_scale of update t = 1 / sqrt(1 - (1 - c_sigma)^(2 t)),
 *                       t from 1); the Adam buffers are not used.  One GPU only: world > 1 is SES_ERR_UNSUPPORTED (sharded runs call
 *                       ses_sepcma_generation per generation).
 *   lm_ps[2], lm_M[2], lm_step[2], lm_weights, lm   SES_STRATEGY_LM_MA_ES only (after the sep_cma_es fields): the path, the direction
 *                       vectors and the step factor as ping-pong halves, the weight table [lm.mu] and the constants of
 *                       ses_lmma_generation; adam_t counts the updates.  One GPU only.
 *   ma_ps[2], ma_M[2], ma_step[2], ma_D[2], ma_weights, ma   SES_STRATEGY_MA_ES only (at the END of the struct): the path
 *                       (float32[P]), the matrix (float32[P, P]), the step factor (float32[1]) and D (float32[n, P]: ma_D[cur] is the D
 *                       of the current population) as ping-pong halves like parents[], the float32 weight table [ma.mu] and the
 *                       constants of ses_maes_generation.  n = offspring_num (>= 4; no mu row), parents = mu[P]; adam_t counts the
 *                       updates; the Adam buffers are not used.  One GPU only: world > 1 is SES_ERR_UNSUPPORTED (sharded runs call
 *                       ses_maes_generation per generation with d_in = NULL).
 *   ars_b               SES_STRATEGY_ARS only (at the END of the struct): b of ses_ars_generation, 1 <= ars_b <= n / 2.  n = offspring_num
 *                       (even, >= 4; no mu row), parents = mu[P], learning_rate as given; no other buffer.  The step is formed on the
 *                       device, so nothing comes back to the host per generation.  One GPU only: world > 1 is SES_ERR_UNSUPPORTED
 *                       (sharded runs call ses_ars_generation per generation).
 * best: float[k], device or PINNED HOST memory (the kernels store straight into it) <- max(fitness) of each generation;
 * stamps: optional uint64[k][2] in device-visible memory <- the GPU's 100 MHz counter at the end of each rollout phase and
 * at the start of the launch that writes the next population (ses_set_stamp).  The handle's own stamp is left as it was.
 */
#define SES_STRATEGY_OPENAI_ES 0        /* offspring_strategies.py:262-434 */
#define SES_STRATEGY_SIMPLE_EVOLUTION 1 /* offspring_strategies.py:128-259 */
#define SES_STRATEGY_SIMPLE_GENETIC 2   /* offspring_strategies.py:11-125  */
#define SES_STRATEGY_PGPE 3             /* ses_perturb_mirrored / ses_pgpe_generation */
#define SES_STRATEGY_SEP_CMA_ES 4       /* ses_perturb_sepcma / ses_sepcma_generation */
#define SES_STRATEGY_LM_MA_ES 5         /* ses_perturb_lmma / ses_lmma_generation */
#define SES_STRATEGY_MA_ES 6            /* ses_perturb_maes / ses_maes_generation */
#define SES_STRATEGY_ARS 7              /* ses_perturb_mirrored (scale = 1) / ses_ars_generation */
typedef struct ses_gen_state {
    int32_t strategy, n, elite_num, mode, shared_init, init_width;
    float init_lo, init_hi;
    uint64_t seed, env_seed;
    double learning_rate, sigma_decay;
    double sigma, pop_sigma;
    uint64_t pop_gen;
    int64_t adam_t;
    int32_t cur, world;
    float *theta[2];
    float *parents[2];
    float *adam_m[2];
    float *adam_v[2];
    int32_t *parent_map;
    int32_t *alias_state;
    float *fitness;
    float *init;
    int32_t *work_i32;
    float *work_f32;
    int64_t first_row;
    int32_t n_local, per_rank;
    ses_handle *comm;
    float *fit_local;
    float *scale[2];
    double sigma_learning_rate, sigma_max_change;
    float scale_lo, scale_hi;
    float *cma_C[2];
    float *cma_ps[2];
    float *cma_pc[2];
    float *cma_step[2];
    const float *cma_weights;
    ses_sepcma_params cma;
    float *lm_ps[2];
    float *lm_M[2];
    float *lm_step[2];
    const float *lm_weights;
    ses_lmma_params lm;
    float *ma_ps[2];
    float *ma_M[2];
    float *ma_step[2];
    float *ma_D[2];
    const float *ma_weights;
    ses_maes_params ma;
    int32_t ars_b, ars_reserved;
} ses_gen_state;
int ses_run_generations(ses_handle *h, ses_gen_state *st, int32_t k, float *best, uint64_t *stamps);

/* ---- multi-GPU: fitness all-gather over RCCL (replaces the gather half of Pool.map, loop.py:66-79) ---------- */
/*
 * The population shards over one process per GPU: rank r of W owns n_per_rank = ceil(N / W) consecutive global
 * rows (the last rank pads its shard, e.g. with -inf).  The ONE exchange of a generation is the all-gather of the
 * float32 fitness shards, N * 4 bytes (16 KB at N = 4096): latency-bound on xGMI, one ncclAllGather, no bucketing.
 * Everything after it (rank shaping, ES update, elite rows) is recomputed identically on every rank from the
 * counter-based noise, so there is no second collective.
 *   ses_comm_unique_id : rank 0 fills id[SES_COMM_ID_BYTES] (ncclGetUniqueId); the host hands the bytes to the other
 *                        ranks by whatever it has (a file, MPI, a torch.distributed store, ...).
 *   ses_comm_init      : collective over the W ranks; binds an RCCL communicator for the handle's device to the handle.
 *   ses_allgather_fitness : all[r * n_per_rank + i] = local_r[i] on every rank, enqueued on the handle's stream.
 * RCCL (librccl.so.1) is loaded on the first ses_comm_* call; single-GPU users never load it.
 */
#define SES_COMM_ID_BYTES 128
int ses_comm_unique_id(void *id);
int ses_comm_init(ses_handle *h, int32_t rank, int32_t world, const void *id);
/* rank / world of the handle's communicator (world = 0: none) and the RCCL version code; any pointer may be NULL */
int ses_comm_info(ses_handle *h, int32_t *rank, int32_t *world, int32_t *rccl_version);
int ses_comm_destroy(ses_handle *h); /* also done by ses_destroy */
int ses_allgather_fitness(ses_handle *h, const float *local, int32_t n_per_rank, float *all);
/*
 * The same exchange by PEER STORES inside one node (no RCCL, no ring): every rank owns a mailbox in fine-grained device
 * memory, the W - 1 peers map it (hipIpc*), and one small kernel per rank stores its shard into every peer's mailbox,
 * publishes a sequence number and collects the peers' shards from its own mailbox -- the latency of one xGMI store
 * instead of W - 1 ring hops behind a library launch.  Once attached, ses_allgather_fitness uses it for n_per_rank <=
 * max_per_rank (results identical: it is a copy).  A wait that exceeds the time-out ("comm_p2p_timeout_ms", default 60 s)
 * NaN-fills the missing shard and sets that peer's bit in a host-visible word: ses_comm_p2p_status reads it at any time
 * without touching the stream (once the kernels that consume an exchange have finished, the word is final for it -- check
 * it before a generation's results are used or checkpointed), and the next ses_allgather_fitness fails with SES_ERR_COMM
 * unless "comm_p2p_keep_going" is set; after ses_comm_p2p_detach the handle is back on RCCL.
 *   ses_comm_p2p_export : allocate this rank's mailbox; handle[SES_COMM_P2P_HANDLE_BYTES] is what the peers need.
 *   ses_comm_p2p_attach : handles = the W exported handles in rank order (W * SES_COMM_P2P_HANDLE_BYTES bytes, gathered
 *                         by the host's control plane); maps the peers.  Every rank must have exported before any attaches.
 *   ses_comm_p2p_info   : world (0 = not attached), max_per_rank, exchanges done so far; any pointer may be NULL.
 * Ranks may share a GPU (several processes on one device): that is how the single-GPU tests drive this path.
 */
#define SES_COMM_P2P_HANDLE_BYTES 64
int ses_comm_p2p_export(ses_handle *h, int32_t rank, int32_t world, int32_t max_per_rank, void *handle);
int ses_comm_p2p_attach(ses_handle *h, const void *handles);
/* The same transport between handles of ONE process (a host that drives several GPUs, or several streams of one GPU, from
 * one process; also how one test process forms worlds of 8 and 16 ranks on a single GPU): every handle exports as above, then
 * attaches the peers' HANDLES -- peers[world] in rank order, peers[rank] == h -- instead of their IPC bytes: nothing is
 * mapped, the peers' mailboxes are addressed directly, so they must live on the same device or on devices the caller has
 * enabled peer access between, and every handle must detach before any of them is destroyed.  An exchange kernel WAITS for
 * kernels of its peers: each handle needs not just a stream but a HARDWARE QUEUE of its own.  Handles on different devices
 * have that by construction; for handles that share a device it is the runtime's choice (GPU_MAX_HW_QUEUES, default 4, and
 * the order in which streams were created) -- two streams on one queue are a dead wait until the time-out -- unless the
 * streams come from ses_stream_create_exclusive below (tests/test_gpu_sharded_tail.py: one process, a stream per rank). */
int ses_comm_p2p_attach_local(ses_handle *h, ses_handle *const *peers);
/* A HIP stream with a hardware queue of its OWN on `device`, for handles that share a device and wait for each other's kernels
 * (above).  The runtime pools the queues of ordinary streams -- GPU_MAX_HW_QUEUES of them per priority, shared round-robin --
 * but a stream created with a CU mask (hipExtStreamCreateWithCUMask) never enters the pool: it always gets a queue created for
 * it.  The mask given here names every CU of the device, so it restricts nothing.  *stream is a hipStream_t for ses_create
 * (and torch.cuda.ExternalStream); ses_stream_destroy ends it.  This is what makes the in-process many-rank rig deterministic
 * (tests/test_gpu_sharded_tail.py); one process per GPU -- the product's way to run -- never needs it. */
int ses_stream_create_exclusive(int32_t device, void **stream);
int ses_stream_destroy(void *stream);
int ses_comm_p2p_info(ses_handle *h, int32_t *world, int32_t *max_per_rank, int32_t *exchanges);
/* exchanges issued over the attached transport so far, by kind: with sequence words (ses_allgather_fitness) / as granules (the
 * exchanges kernels do themselves: chunk partials and, inside ses_run_generations, the fitness; the granule all-gather) */
int ses_comm_p2p_counts(ses_handle *h, int32_t *flag_exchanges, int32_t *granule_exchanges);
int ses_comm_p2p_status(ses_handle *h, uint32_t *timed_out_mask);   /* bit r: an exchange gave up waiting for rank r */
/* Clears the time-out mask (drains the handle's stream first): for a host that has dealt with a failed exchange and whose ranks
 * have AGREED to go on using this transport -- e.g. after a failed check of the granule exchanges at attach time, which switches
 * those off ("comm_granules_enabled" = 0) and keeps the flag-based exchanges. */
int ses_comm_p2p_reset_status(ses_handle *h);
int ses_comm_p2p_detach(ses_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* SES_H_ */
