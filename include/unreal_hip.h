/* libunreal_hip.so -- C ABI of the MI355X (gfx950) UNREAL actor-learner hot path.
 *
 * The reference (kvas7andy/unreal, /root/reference) has no FFI of its own: the path sits behind a
 * Python class surface and, below it, TensorFlow's op registry.  Every entry point here replaces one
 * reference call site (cited per function, file:line under /root/reference) and is what a binding
 * for that call would bind.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  ALL pointers are DEVICE pointers owned by the caller
 *     (the Python host allocates them through PyTorch-ROCm); nothing is allocated or freed here.
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream.
 *   - return 0 = OK, -22 = invalid argument (nothing launched), -5 = launch failure.  Never throws.
 *   - No global state apart from a thread-local label of the calling thread's last launch
 *     (unreal_last_launch); not thread-safe per buffer (one host thread per GPU by contract).
 *   - Frames are uint8 NHWC 84x84x3 (21,168 B); a "frame index" f addresses frames + f*21168.
 *   - Ring: actor b owns H1 = H+1 slots; absolute frame i lives in slot i % H1; per-slot metadata
 *     arrays are [B][H1]; the current observation of actor b is slot count[b] % H1.
 */
#ifndef UNREAL_HIP_H
#define UNREAL_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UNREAL_FRAME_BYTES 21168
#define UNREAL_PC_CELLS 400
/* unreal_gemm_f32 flags */
#define UNREAL_GEMM_RELU 1
#define UNREAL_GEMM_ACCUM 2
#define UNREAL_GEMM_ATOMIC 4
#define UNREAL_GEMM_RELU_MASK 8
#define UNREAL_GEMM_RELU_BITS 16   /* split_nt only: mask = uint16 bit words (unreal_encoder_fwd relu_bits), ldm in words */

/* ---- environment (environment/maze_environment.py:50-55,98-128; environment/environment.py:88-102;
 *      train/experience.py:63-93 add_frame; train/trainer.py:194-205,264-296 reset rules) ----------
 * The maze (csrc/maze.hip).  Every maze entry ends in the same maze tail (view, N, cfg, actor_base, goal, layout,
 * ep_steps, episode, heading), in one of four forms:
 *   view 0, cfg NULL   the reference's 7 x 7 map, top-down (N must be 7; goal .. heading are not used)
 *   view 0, cfg block  a configured maze, top-down (environment/maze_environment.py MazeConfig)
 *   view 1, cfg block  a configured maze in first person (MazeConfig(view="first_person")); cfg NULL is EINVAL
 *   view 2, cfg block  a generated maze in first person (MazeConfig(generate=N)); cfg or heading NULL is EINVAL,
 *                      and so is a layout array: a generated block has no layout records, layout must be NULL
 * `cfg` is the configuration block (int32 words: N, layouts, flags, max_episode_steps, seed, start heading + 1; per
 * layout the wall bits, S / G cells and free-cell list); with a block, goal[2B] (x, y), layout[B], ep_steps[B] and
 * episode[B] (-1 before the first reset) are the per-actor state of the configured maze and are required, and so is
 * heading[B] (0: +x, 1: +y, 2: -x, 3: -y) in first person.  N in {7, 12, 14, 21} must be the block's grid size (word 0):
 * the block lives in device memory, so the entry cannot read it, and a kernel whose N differs from the block's writes
 * nothing at all (no frame, no state) rather than index a frame with the wrong cell size -- the call still returns 0.
 * Reset draws are Philox4x32-10 with key = the block's seed and counter = (actor_base + b, episode, 0x4D415A45, 0); word 2
 * draws the first-person start heading when the block's word 7 is 0.
 * First person: actions 0 turn left, 1 turn right, 2 step forward, 3 step back; frames are the raycast 84 x 84 RGB view
 * (bytes 0..255, read at scale 1/255) and r_pc is the pixel change of the two frames over 48 * 255, as
 * unreal_pixel_change_u8.  `frames` must be 16-byte aligned; every pointer an entry writes through is required.
 * Navigation (first person, flag 8 in the block's word 2): after the last layout record the block holds
 * [goal reward, apple reward, hit reward, mode (1: goal_respawn, 2: Lab's six actions), 0, 0, 0, 0] and per layout 65
 * words [n apples <= 64, apple cells ascending, 0 ...].  `heading` then addresses B records of UNREAL_MAZE_NAV_RECORD
 * int32: (heading, apple bits lo, apple bits hi, goals_total, apples_total, 0, 0, 0); apple bit k (the k-th apple cell of
 * the layout) set = collected in the running episode; goals_total / apples_total count from the actor's first reset and
 * no reset zeroes them.  Lab's actions: 0 / 1 look left / right, 2 / 3 strafe left / right (-r / +r), 4 / 5 forward /
 * back.  With goal_respawn a goal is not terminal: the actor moves to S or a free cell other than the goal drawn with
 * counter = (actor_base + b, episode, 0x4D415A52, goals_total), word 1, heading word 2 (or the block's fixed one).
 * Generated (first person, flag 16 in the block's word 2, view 2): the block has 0 layouts and no records;
 * word 6 is still 18 + N * N, and after the header come [goal reward, apple reward, hit reward, mode, gen_loops,
 * gen_apples, 0, 0] (the rewards and mode are read only with flag 8).  `heading` addresses B records of
 * UNREAL_MAZE_GEN_RECORD(N) int32: the 8 navigation words above, then the actor's own layout record (wall bits, S = G =
 * -1, n_free, -1, free cells ascending; 18 + N * N words) and apple record (65 words).  Every reset, the reset entry's
 * and a step's terminal reset alike, first rewrites the two records for the new episode: rooms at the even cells, R =
 * (N + 1) / 2 per side; edge e between neighbouring rooms (horizontal first, row-major: e = j (R - 1) + i, cell (2i + 1,
 * 2j); then vertical: e = R (R - 1) + j R + i, cell (2i, 2j + 1)) has the key (w << 8) | e with w = word e & 3 of the
 * draw with counter (actor_base + b, episode, 0x4D415A47, e >> 2); open are the minimum spanning tree of the room grid
 * under these keys and the gen_loops lightest other edges; apples lie in the gen_apples rooms r = j R + i with the
 * smallest keys (w << 8) | r from counter (actor_base + b, episode, 0x4D415A41, r >> 2).  Goal, start and heading are
 * then drawn over that record as for any block.  A view-1 launch on a generated block, a view-2 launch on any other
 * block and a top-down launch on a generated block write nothing, as a launch with the wrong N.
 * Styled walls (first person, flag 32 in the block's word 2): after everything above the block holds the
 * style section: [S styles (1..7), gen_landmark_density (0..256), 0 x 6], then 8 style words r | g << 8 | b << 16 |
 * pattern << 24 (word k - 1: style k; unused slots and the eighth 0), then, for a static block, per layout
 * UNREAL_MAZE_STYLE_WORDS(N) words of 4-bit style ids: cell c = y * N + x is nibble c & 7 of word c >> 3 (0: a free cell,
 * or a wall that looks as without the flag).  A ray whose first blocked cell is an interior wall of style k >= 1 leaves
 * that style's (r, g, b) in channels 0..2, each channel halved where bit u of the pattern is set (u in 0..7: the eighth
 * of the cell's face that was hit, in world coordinates) and then scaled by 5 / 8 on a face crossed along y.  A generated
 * styled block (flags 16 | 32) has no id words in the block: `heading` then addresses B records of
 * UNREAL_MAZE_GEN_STYLED_RECORD(N) int32, the generated record followed by the actor's id words, which every reset
 * draws once the walls are known: wall cell c with w = word c & 3 of the draw with counter (actor_base + b, episode,
 * 0x4D415A53, c >> 2) is a landmark iff (w >> 24) < gen_landmark_density, of style 1 + (w & 0xFFFFFF) % S.  The entries
 * and the view values are the same; the flag selects the styled path, and a launch with the wrong N still writes
 * nothing.
 * Goal sense (first person, flag 64 in the block's word 2, always with flag 8; views 3 and 4): words 5, 6, 7
 * of the 8 navigation words hold gf, gs and d of the actor's current state: gf = (gx - x) dx + (gy - y) dy and gs =
 * (gx - x) rx + (gy - y) ry, the goal's offset along the heading's forward axis d and right axis r, and d the path distance
 * of the actor's cell: the length of the shortest 4-connected path over free cells to the episode's goal.  Every record
 * ends in the actor's distance field, UNREAL_MAZE_DIST_WORDS(N) int32: cell c = y * N + x is the 16-bit half c & 1 of word
 * c >> 1; wall cells, and the unused half of the last word where N * N is odd, hold 0xFFFF.  `heading` addresses B records
 * of UNREAL_MAZE_SENSE_RECORD(N) int32 (a static block, view 3) or of UNREAL_MAZE_GEN_RECORD(N) / ..._GEN_STYLED_RECORD(N)
 * + UNREAL_MAZE_DIST_WORDS(N) (a generated block, view 4).  The field is computed by a breadth-first search at every
 * reset, the reset entry's and a step's terminal reset alike, after the goal is drawn (generated: after the layout is
 * written); a respawn at the goal keeps it.  Word 6 of the navigation header is progress_reward p: a step's reward is the
 * first-that-applies reward plus p * (d of the cell before the action - d of the cell the move ends in, before any respawn
 * or reset).  A launch of view 3 / 4 on a block without the flag, or of view 1 / 2 on a block with it, writes nothing.
 * unreal_maze_objective turns words 5..7 into the ring's objective vectors.
 * Foraging (first person, flag 128 in the block's word 2, always with flag 8 and never with flag 64; views 5 and 6;
 * DESIGN §7j): up to three more kinds of pickup next to the apple, and episodes without a goal.  The block ends, after
 * everything above, in 16 words: [0] K kinds (0..3)  [1] mode (bit 0: no goal)  [4..6] the rewards of kinds 1..3  [8..10]
 * r | g << 8 | b << 16 | ends_episode << 24 of kinds 1..3  [12..14] gen_pickups (rooms of a generated maze that hold kind
 * 1..3, ranked after the gen_apples rooms by the same keys); every other word 0.  Entry k of an apple record, the block's
 * or a generated actor's, is cell | kind << 16, ascending by cell (kind 0: the apple, with the navigation header's apple
 * reward and floor colour (40, 255, 40)); bit k of the actor's collected mask is entry k.  A move into the cell of an
 * active pickup pays its kind's reward (after the goal's, before a hit's) and, for a kind with ends_episode, ends the
 * episode, also under goal respawn; the floor of an active pickup's cell has its kind's colour.  Words 4..7 of the 8
 * navigation words are the running totals of kinds 0..3, never zeroed.  Without a goal, goal[] holds (-1, -1), a layout
 * record's G is -1, and the start is S or free cell number (word 1 of the reset draw) % n_free.  The record widths are
 * those of views 1 and 2.  A launch of view 5 / 6 on a block without the flag, or of any other view on a block with it,
 * writes nothing. */
#define UNREAL_MAZE_NAV_RECORD 8
#define UNREAL_MAZE_GEN_RECORD(N) (8 + 18 + (N) * (N) + 65)
#define UNREAL_MAZE_STYLE_WORDS(N) (((N) * (N) + 7) / 8)
#define UNREAL_MAZE_GEN_STYLED_RECORD(N) (UNREAL_MAZE_GEN_RECORD(N) + UNREAL_MAZE_STYLE_WORDS(N))
#define UNREAL_MAZE_TOP_DOWN 0
#define UNREAL_MAZE_FIRST_PERSON 1
#define UNREAL_MAZE_FIRST_PERSON_GENERATED 2
#define UNREAL_MAZE_DIST_WORDS(N) (((N) * (N) + 1) / 2)
#define UNREAL_MAZE_SENSE_RECORD(N) (8 + UNREAL_MAZE_DIST_WORDS(N))
#define UNREAL_MAZE_FIRST_PERSON_SENSE 3
#define UNREAL_MAZE_FIRST_PERSON_GENERATED_SENSE 4
#define UNREAL_MAZE_FIRST_PERSON_FORAGE 5
#define UNREAL_MAZE_FIRST_PERSON_GENERATED_FORAGE 6
/* env.reset() of every actor where mask[b] != 0 (mask nullable) */
int unreal_maze_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward, const int* count,
                      uint8_t* frames, int view, int N, const int* cfg, int actor_base, int* goal, int* layout,
                      int* ep_steps, int* episode, int* heading, void* stream);
/* environment.process + experience.add_frame of every actor where active[b] != 0 (active, out_reward, out_terminal
 * nullable; episode_reward / score_out / score_valid required with track_score) */
int unreal_maze_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action, float* last_reward,
                     int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                     float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                     float* score_out, int* score_valid, int reset_on_terminal, int track_score, int view, int N,
                     const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps, int* episode, int* heading,
                     void* stream);
/* the same step with the rollout loop's bookkeeping (train/trainer.py:236-296) in the same launch: `active` is read
 * AND updated (an actor leaves the rollout at its terminal, the reference's `break`), active_log_t / n_steps /
 * terminal_end as unreal_rollout_advance writes them, next_idx = ring index of every actor's next observation
 * (unreal_ring_cur_idx) and next_lar = the [one-hot last action | last reward] columns of the next step's LSTM-input
 * rows (unreal_lar_fill): three ~5 us launches per rollout step less.  reset_on_terminal = track_score = 1. */
int unreal_maze_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward, int* count,
                             uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                             float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                             float* episode_reward, float* score_out, int* score_valid, int* active, int* active_log_t,
                             int* n_steps, int* terminal_end, int* next_idx /*nullable*/, float* next_lar /*nullable*/,
                             int lar_ld, int lar_col0, int A,
                             int idx_base_actor /* next_idx[b] = (idx_base_actor + b) * H1 + slot: a half-batch whose
                                                   rows index the whole ring */,
                             int view, int N, const int* cfg, int actor_base, int* goal, int* layout, int* ep_steps,
                             int* episode, int* heading, void* stream);
/* unreal_policy_step + unreal_maze_rollout_step in ONE launch (trainer.py:236-296: run_base_policy_and_value, choose_action,
 * environment.process of one rollout step): the workgroup that steps an actor first computes its pi / V from the feature row
 * X[b] (K = 256) and draws its action from u[b] -- bit-identical to the two-launch path.  A must be 4 (the maze), or 6 on a
 * first-person navigation block with Lab's actions; a first-person launch whose A is not its block's action count
 * writes nothing (as a block of another N). */
int unreal_maze_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                    const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                    int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                    uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action,
                                    float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                    float* episode_reward, float* score_out, int* score_valid, int* active,
                                    int* active_log_t, int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                                    float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                    int view, int N, const int* cfg, int actor_base, int* goal, int* layout,
                                    int* ep_steps, int* episode, int* heading, void* stream);
/* The wall image of every layout of a top-down block (cfg NULL: of the reference's map, N = 7, n_templates = 1):
 * templates[l * 21168 ..) = the frame of layout l with channel 0 = 1 in wall cells and everything else 0 -- the frame the
 * maze kernels draw before the agent and goal blocks (maze_environment.py:57-74 _get_current_image without the two
 * blocks).  Layouts do not change once a block is bound, so this runs once per block.  n_templates must be the block's
 * layout count (word 1; another count writes nothing); templates 16-byte aligned.  (csrc/maze.hip) */
int unreal_maze_wall_templates(int N, const int* cfg, int n_templates, uint8_t* templates, void* stream);
/* unreal_maze_policy_rollout_step + unreal_encoder_fwd of the NEXT observations in ONE launch (csrc/rollout_fused.hip;
 * trainer.py:236-296 environment.process, then model.py:281-289 on the next step's states): the workgroup that steps actors
 * 8w .. 8w + 7 builds each 16-byte piece of their next frames in registers (the layout's template from
 * unreal_maze_wall_templates + the agent and goal blocks), stores it to the ring slot and expands the same registers into
 * the encoder's image, so the frame is never read back.  Row b of c1_out / f2_out / relu_bits is the encoding of actor b's
 * next observation, the frame next_idx[b] names; an idle actor's comes from its ring slot.  Everything the two launches
 * write is written, bit for bit.  Top-down only (view 0), A = 4, cfg NULL or a block; `prepared` (unreal_encoder_prepare
 * for frame_scale), c1_out, relu_bits and templates are required; anything else is -EINVAL.  A block of another N or
 * layout count than N / n_templates writes nothing.  `heading` is not used. */
int unreal_maze_policy_rollout_step_encode(
    int B, int H1, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv, const float* bv,
    const double* u, float* pi_out, float* v_out, int* actions_out, int* pos, int* last_action, float* last_reward,
    int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
    float* r_pc, float* out_reward, int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
    int* active, int* active_log_t, int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
    float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A, int idx_base_actor, int view, int N, const int* cfg,
    int actor_base, int* goal, int* layout, int* ep_steps, int* episode, int* heading, const uint8_t* templates,
    int n_templates, float frame_scale, const float* W1, const float* b1, const float* W2, const float* b2, float* c1_out,
    float* f2_out, uint16_t* relu_bits, float* f2_absmax /*nullable*/, float* c1_absmax /*nullable*/, const void* prepared,
    void* stream);
/* Time-limit bootstrapping: the two rollout entries above with a final-observation store, for the
 * first-person views without goal sense (views 1, 2, 5, 6; any other view: -EINVAL).  A step is a TRUNCATION when the
 * episode ends in it only because of the step limit: steps >= max_episode_steps, no ending pickup, and no goal reached
 * unless goals respawn (then a goal in that step is no end).  A truncation writes s_{t+1}, the observation the limit cut
 * off, to final_obs[b] (one 21168-byte frame per actor of the launch) before the next episode's first view goes to the ring
 * slot, and commits 2 instead of 1 to r_terminal[slot], out_terminal[b] and terminal_end[b]; every consumer of these words
 * tests them for non-zero.  A true end writes 1 and leaves final_obs[b] alone.  Everything else is written as by the
 * entries above.  -EINVAL also for a null final_obs or one not 16-byte aligned. */
int unreal_maze_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                float* episode_reward, float* score_out, int* score_valid, int* active, int* active_log_t,
                                int* n_steps, int* terminal_end, int* next_idx /*nullable*/, float* next_lar /*nullable*/,
                                int lar_ld, int lar_col0, int A, int idx_base_actor, int view, int N, const int* cfg,
                                int actor_base, int* goal, int* layout, int* ep_steps, int* episode, int* heading,
                                uint8_t* final_obs, void* stream);
int unreal_maze_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                       const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                       int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                       uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                       int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                       int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                       int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                       int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld, int lar_col0,
                                       int A, int idx_base_actor, int view, int N, const int* cfg, int actor_base,
                                       int* goal, int* layout, int* ep_steps, int* episode, int* heading,
                                       uint8_t* final_obs, void* stream);
/* The objective vectors of a goal-sense maze, from the per-actor records the maze entries keep behind
 * `heading` (record_words int32 each, >= 8): for every actor b, {w5 / 32, w6 / 32, w7 / 512} of record b go to
 * r_objective[(b * H1 + count[b] % H1) * 3 ..), the slot of the actor's current observation, and, with next_lar, to
 * next_lar[b * lar_ld + lar_col0 .. + 3), the objective columns of the next step's LSTM-input row.  Nothing else is
 * written; a second call writes the same values.  -EINVAL without a launch: B <= 0, H1 <= 0, record_words < 8, a null
 * count / records / r_objective, or next_lar with lar_col0 < 0 or lar_ld < lar_col0 + 3. */
int unreal_maze_objective(int B, int H1, const int* count, const int* records, int record_words, float* r_objective,
                          float* next_lar /*nullable*/, int lar_ld, int lar_col0, void* stream);
/* Depth labels of first-person mazes (csrc/depth.hip): the depth class of UNREAL_DEPTH_POSITIONS columns of
 * every actor's current view, computed from its cell, heading and walls in integers.  Position j is frame column
 * i = 7 j + 3 (q = 2 i + 1 - 84, odd); its ray is the camera's (above): t = tn / td at the first wall cell or map border,
 * a border like any wall.  The class, 0 .. UNREAL_DEPTH_CLASSES - 1, is the number of edges e in {1, 2, 3, 4, 6, 8, 12}
 * with tn >= e td, so a ray that ends exactly on an edge is in the upper class.  Pickups, the goal and wall styles do not
 * change it.  The 12 bytes go to r_depth[(b * H1 + count[b] % H1) * 12 ..), the slot of the actor's current observation
 * (the slot unreal_maze_objective writes); nothing else is written and a second call writes the same bytes.
 * pos[2B], cfg and layout are the maze tail's; `heading` is the tail's heading argument: heading[B] with record_words 0,
 * or the B per-actor records of record_words int32 (word 0: the heading).  layout NULL: a generated block, whose wall
 * bits are read from the actor's record (record_words >= UNREAL_MAZE_GEN_RECORD(N)).  Every first-person view is served
 * (plain, generated, goal sense, forage; styled or not).  A launch whose N is not the block's, or with a layout array on
 * a generated block (or none on a static one), writes nothing.  -EINVAL without a launch: B <= 0, H1 <= 0, N not in
 * {7, 12, 14, 21}, a null count / pos / heading / cfg / r_depth, record_words < 0 or in 1..7, or layout NULL with a
 * record shorter than the generated record. */
#define UNREAL_DEPTH_POSITIONS 12
#define UNREAL_DEPTH_CLASSES 8
int unreal_maze_depth_labels(int B, int H1, int N, const int* count, const int* pos, const int* heading, int record_words,
                             const int* cfg, const int* layout /*nullable*/, uint8_t* r_depth, void* stream);
/* Device arcade (csrc/arcade.hip): games stepped and rendered on the device, one actor per workgroup.  The
 * four entries take the ring and rollout arguments of the maze entries above (`pos` is accepted and never touched;
 * nullable) and commit through the same helpers; the maze tail is replaced by (cfg, actor_base, ep_steps[B], episode[B],
 * records[B][UNREAL_ARCADE_RECORD]).  There is one launch shape and no launch label.
 *
 * cfg: UNREAL_ARCADE_CFG_WORDS int32 words; word 0 is the game id, which the kernels read from the block (uniform):
 * UNREAL_ARCADE_BREAKOUT, UNREAL_ARCADE_DUEL, UNREAL_ARCADE_INVADERS or UNREAL_ARCADE_CROSSING (below); a kernel that reads
 * another id (0, 2, 4 and negative ones included) writes nothing.
 * Breakout's block: [0] UNREAL_ARCADE_BREAKOUT  [1] action_repeat - 1, 0..7 (the kernel clamps it; see "An agent step"
 * below)  [2] rows 1..6  [3] max_episode_steps >= 1  [4..5] seed (lo, hi)  [6] paddle_width (even, 4..24)
 * [7] paddle_speed 1..8  [8] ball_speed 1..4  [9] lives 1..5  [10] serve_wait 0..255 (0: only fire serves)
 * [11] life_reward -100..0  [12..17] row rewards 0..100, top row first  [18] return_reward 0..100  [19..23] 0.
 * record: [0..6] px, bx, by, vx, vy, wait (>= 0: the ball waits to be served, -1: in flight), lives  [7..8] live bricks
 * (bit 10 r + c, lo, hi)  [9] serve_index  [10] bricks total  [11] lives-lost total  [12] walls-cleared total (the totals
 * are never zeroed)  [13..15] 0.
 *
 * Breakout, actions 0 noop, 1 fire, 2 right, 3 left (ALE's minimal set: A = 4).  Frame 84 x 84 x 3 bytes (frame scale
 * 1 / 255), back to front: black; border (142, 142, 142) on rows 0..5 and columns 0..1, 82..83; life k < lives the block
 * x 4+4k..5+4k, y 2..3 in (236, 236, 236); brick (r, c) x 2+8c..9+8c, y 18+3r..20+3r in its row's colour; paddle y 78..79,
 * x px..px+w-1 in (200, 72, 72); the ball, 2 x 2 at (bx, by) in (236, 236, 236), only in flight.  One tick (with
 * action_repeat = 1 an agent step is one tick; steps += 1 and rule 4 belong to the agent step, see below):
 *  1. steps += 1; action 2 / 3 moves the paddle by paddle_speed, clamped to [2, 82 - w].
 *  2. A waiting ball is served on fire, or when serve_wait > 0 and wait >= serve_wait: u = Philox4x32-10(key = seed,
 *     counter = (actor_base + b, episode, 0x41524B53, serve_index)); bx = 2 + 2 (u[0] % 39), by = 40, vx = u[1] & 1 ? +1
 *     : -1, vy = +1, wait = -1, serve_index += 1.  Otherwise wait += 1.  The ball does not move in such a step.
 *  3. A ball in flight makes ball_speed micro-steps, each an x move and then a y move, ending early after the micro-step
 *     in which a life is lost or the last brick goes.  x: tx = bx + vx; outside [2, 80]: vx = -vx; else if the 2 x 2 box at
 *     (tx, by) overlaps live bricks: the one with the lowest bit is cleared and pays its row's reward, vx = -vx; else
 *     bx = tx.  y: ty = by + vy; ty < 6: vy = +1; else a brick as in x (vy = -vy); else if vy > 0, ty + 1 == 78 and
 *     [bx, bx+1] meets the paddle: vy = -1 and, with d = bx + 1 - (px + w / 2), vx = -2 if 4 d < -w, -1 if d < 0, +1 if
 *     4 d < w, else +2, and the reward gets return_reward; else if ty + 1 > 83: lives -= 1, the reward gets life_reward,
 *     wait = 0; else by = ty.
 *  4. terminal: lives <= 0, no live brick, or steps >= max_episode_steps.  With reset_on_terminal the next episode starts
 *     (episode += 1, full wall, all lives, px = 42 - w / 2, ball waiting, wait = serve_index = steps = 0) and its first
 *     frame goes into the next slot.  The pixel change is that of the two frames before the reset, over 48 * 255.
 *
 * An agent step (every game).  With word 1 = k - 1 one call of a step entry is one agent step of up to k
 * ticks:
 *  a. A tick is rules 1..3 above (the duel: its rules 1..4) without `steps += 1`, every tick with the step's action: the
 *     paddle moves in every tick, so does the duel's opponent (from the ball of the state before that tick); a repeated
 *     fire serves while the ball waits and is a noop in flight; `wait` advances once per tick; a ball served in one tick
 *     flies in the next, and a lost life or point can be followed by waiting ticks and the next serve, all in one step.
 *  b. The ticks stop after a tick that ends the game by the state's own conditions (Breakout: lives <= 0 or no live
 *     brick; duel: mine >= points or theirs >= points).  Without reset_on_terminal the state stays ended, so every later
 *     step runs exactly one tick.
 *  c. steps, max_episode_steps, ep_steps and the ring count agent steps, not ticks, and the step limit never shortens a
 *     step's ticks.  terminal is rule 4 (the duel: 5) on the record after the last tick run and the agent step count;
 *     the endings keep their order.
 *  d. The step's reward is the sum over its ticks, raw and unclipped into last_reward and the ring.
 *  e. Word 18, return_reward, is added in the tick in which the AGENT's paddle returns the ball (Breakout: the
 *     ty + 1 == 78 branch; duel: branch (a)); the opponent's returns pay nothing.  A tick holds at most one such return.
 *  f. The frame stored is the render of the record after the last tick, and the pixel change is between that frame and
 *     the frame before the step: the states between ticks are never drawn.  The kernel finds the rows that can differ
 *     from the two end records alone, which stays exact for any k because it compares only fields that are drawn.
 *  g. Serve draws keep their key and counter (seed, global actor, episode, serve_index): no other random stream.
 * At word 1 = 0 and word 18 = 0 every entry computes what it computed before these words had a meaning.
 *
 * The duel (UNREAL_ARCADE_DUEL): Breakout's field, ball, serve draw and four actions, with an opponent's paddle
 * in place of the wall.  cfg: [0] UNREAL_ARCADE_DUEL  [1] action_repeat - 1, 0..7  [2] points 1..9
 * [3] max_episode_steps >= 1  [4..5] seed (lo, hi)  [6] paddle_width (even, 4..24)  [7] paddle_speed 1..8  [8] ball_speed 1..4  [9] opponent_width (even, 4..24)
 * [10] serve_wait 0..255  [11] lose_reward -100..0  [12] win_reward 0..100  [13] opponent_speed 0..8 (0: it stands)
 * [14..17] 0  [18] return_reward 0..100  [19..23] 0.
 * record: [0..5] px, bx, by, vx, vy, wait  [6] ox  [7] mine  [8] theirs (the two scores)  [9] serve_index  [10] points-won
 * total  [11] points-lost total  [12] matches-won total (the totals are never zeroed)  [13..15] 0.
 * Frame, back to front: black; Breakout's border; score blocks on rows 2..3: the agent's k-th point (k = 0..) x 4+4k..5+4k
 * in (236, 236, 236), the opponent's k-th x 78-4k..79-4k in (66, 72, 200), nine of each at the most; the agent's paddle
 * y 78..79, x px..px+paddle_width-1 in (200, 72, 72); the opponent's y 8..9, x ox..ox+opponent_width-1 in (66, 72, 200);
 * the ball as in Breakout, only in flight.  One tick (an agent step is up to action_repeat ticks: "An agent step" above):
 *  1. steps += 1; the agent's paddle as in Breakout.
 *  2. The opponent's paddle, from the ball of the state before this step: target = bx + 1 if the ball is in flight and
 *     vy < 0, else 42; d = target - (ox + opponent_width / 2); ox += clamp(d, -opponent_speed, +opponent_speed), then
 *     clamped to [2, 82 - opponent_width].  It moves in every step, also while the ball waits.
 *  3. A waiting ball is served as in Breakout (same key and counter words, bx, by = 40, vx), and vy = u[2] & 1 ? +1 : -1.
 *  4. A ball in flight makes ball_speed micro-steps, each an x move and then a y move; a point ends them.  x: tx = bx + vx;
 *     outside [2, 80]: vx = -vx; else bx = tx.  y: ty = by + vy, tested in this order: (a) vy > 0, ty + 1 == 78 and
 *     [bx, bx+1] meets the agent's paddle: vy = -1, Breakout's vx from d = bx + 1 - (px + paddle_width / 2) and the
 *     reward gets return_reward; (b) vy < 0,
 *     ty == 9 and [bx, bx+1] meets the opponent's: vy = +1, vx by the same rule from ox and opponent_width; (c) ty + 1 > 83:
 *     theirs += 1, the reward gets lose_reward, wait = 0; (d) ty < 6: mine += 1, the reward gets win_reward, wait = 0;
 *     (e) else by = ty.  A point leaves bx, by, vx, vy as they are.
 *  5. terminal: mine >= points, theirs >= points, or steps >= max_episode_steps.  Matches-won counts the step in which
 *     mine reaches points, once.  With reset_on_terminal the next episode starts (episode += 1, px = 42 - paddle_width / 2,
 *     ox = 42 - opponent_width / 2, bx = by = vx = vy = wait = mine = theirs = serve_index = steps = 0).  Without it the
 *     game goes on: the scores run past points and terminal stays set.
 *
 * Invaders (UNREAL_ARCADE_INVADERS): a fixed shooter on Breakout's field, border, life blocks and four actions
 * (0 noop, 1 fire, 2 right, 3 left).  cfg: [0] UNREAL_ARCADE_INVADERS  [1] ticks per agent step less one, 0..7, as above  [2] alien_rows 1..4
 * (the kernel clamps it)  [3] max_episode_steps >= 1  [4..5] seed (lo, hi)  [6] paddle_width, the cannon's (even, 4..24)
 * [7] paddle_speed 1..8  [8] ball_speed, the shot's, 1..4 (clamped)  [9] lives 1..5  [10] serve_wait 0..255, the grace
 * [11] life_reward -100..0  [12..15] alien rewards 0..100, top row first  [16] march_period 1..16  [17] descend 1..8
 * [18] return_reward, 0 (no paddle returns a ball; never read)  [19] bomb_period 1..64  [20] bomb_speed 1..4 (clamped)
 * [21..23] 0.
 * record: [0] px  [1..2] sx, sy, the shot (sy = 0: none; in flight 6 <= sy <= 76)  [3..4] gx, gy, the grid's origin
 * [5] direction +1 / -1  [6] lives  [7] live aliens (bit 8 r + c)  [8] march counter | bomb counter << 8 | grace counter
 * << 16  [9] draw_index  [10] aliens-shot total  [11] lives-lost total  [12] waves-cleared total (the totals are never
 * zeroed)  [13..15] the three bombs, x | y << 8 (0: the slot is free).
 * Frame, back to front: black; Breakout's border and life blocks; alien (r, c), r < alien_rows, c < 8, x gx+8c..gx+8c+5,
 * y gy+6r..gy+6r+3 in Breakout's colour of brick row r; the cannon y 78..79, x px..px+paddle_width-1 in (200, 72, 72); the
 * bombs, 2 x 2 at (x, y) in (214, 214, 92), slot 2 behind slot 1 behind slot 0; the shot, 2 x 2 at (sx, sy) in
 * (236, 236, 236).  One tick (an agent step is up to action_repeat ticks: "An agent step" above, where the game ends by
 * its own conditions with lives <= 0 or no live alien):
 *  1. steps += 1; action 2 / 3 moves the cannon by paddle_speed, clamped to [2, 82 - paddle_width]; action 1 with no shot
 *     in flight starts one at (px + paddle_width / 2 - 1, 76); with a shot in flight it is a noop.
 *  2. A shot (one fired in step 1 included) makes ball_speed micro-steps: sy -= 1; if sy < 6 the shot is removed; else if
 *     the 2 x 2 box at (sx, sy) overlaps live aliens, the one with the lowest bit is cleared and pays its row's reward, the
 *     aliens-shot total grows (and the waves-cleared total if it was the last), and the shot is removed.  A removed shot
 *     has sx = sy = 0 and ends the micro-steps.
 *  3. march += 1; at march >= march_period: march = 0 and the grid moves: nx = gx + 2 direction; if nx is outside 2..20:
 *     gy = min(gy + descend, 84), direction = -direction, gx stays; else gx = nx.
 *  4. The bombs in slot order, each bomb_speed micro-steps: y += 1; if y + 1 > 83 the bomb is removed; else if [x, x+1]
 *     meets [px, px+paddle_width-1] and [y, y+1] meets [78, 79]: lives -= 1, the lives-lost total grows, the reward gets
 *     life_reward, the shot and all three bombs are removed, grace = serve_wait + 1, and the step 4 of this tick ends.
 *     Shot and bombs do not interact.
 *  5. If grace > 0: grace -= 1 and no bomb is dropped in this tick.  bomb += 1; at bomb >= bomb_period: bomb = 0 and, if
 *     the grace allows, an alien lives and a slot is free (the first free one is taken): u = Philox4x32-10(key = seed,
 *     counter = (actor_base + b, episode, 0x494E5642, draw_index)), draw_index += 1; of the columns that hold a live
 *     alien, in ascending order, number u[0] % (their count) is c; r is the row of its lowest live alien; the bomb starts
 *     at (gx + 8 c + 2, gy + 6 r + 4) and first moves in the next tick.  Otherwise no draw is made.
 *  6. If the grid moved in step 3, lives > 0, an alien lives and gy + 6 r + 3 >= 76 for the row r of the lowest live alien:
 *     the invasion: the reward gets life_reward once, the lives-lost total grows by lives, lives = 0.
 *  7. terminal: no live alien (the wave is cleared: success), lives <= 0, or steps >= max_episode_steps.  With
 *     reset_on_terminal the next episode starts (episode += 1, px = 42 - paddle_width / 2, no shot, no bomb, gx = gy = 10,
 *     direction = +1, all lives, the full grid, march = bomb = draw_index = steps = 0, grace = serve_wait).  Without it
 *     the game goes on: lives fall below 0, the grid marches on (gy stops at 84), terminal stays set.
 *
 * Crossing (UNREAL_ARCADE_CROSSING): a walker crosses up to eight lanes of traffic from the bottom of Breakout's
 * field to its top; the reward is sparse.  Actions: 0 noop, 1 forward (up the screen), 2 right, 3 left (A = 4).
 * cfg: [0] UNREAL_ARCADE_CROSSING  [1] ticks per agent step less one, 0..7, as above  [2] lanes L 1..8 (the kernel clamps it)
 * [3] max_episode_steps >= 1  [4..5] seed (lo, hi)  [6] paddle_width, the walker's (even, 4..24)  [7] paddle_speed, its
 * lateral speed, 1..8  [8] ball_speed, its forward speed, 1..4 (clamped)  [9] crossings 0..99, the episode's target (0:
 * none, a purely timed game)  [10] serve_wait 0..255, the stun after a hit  [11] hit_reward -100..0  [12] cross_reward
 * 0..100  [13] knock_back 1..70  [14] car_length 4..16 (clamped to 0..16)  [18] return_reward, 0 (never read)  [20..23] 0,
 * and the lanes' four settings as bit fields, one word per setting over all eight lanes (lane l = 0 is the top one; the
 * fields of lanes >= L are 0):  [15] log2(cars) at bit 2 l (cars 1, 2 or 4; the code 3 reads as 4)  [16] speed 0..4 at
 * bit 3 l (0: parked; above 4 reads as 4)  [17] period - 1 at bit 2 l (period 1..4)  [19] bit l: the lane moves to the
 * right (direction +1), else to the left.
 * record: [0..1] px, py, the walker  [2] stun  [3] crossings of the episode  [4] tick counter, the ticks of the episode
 * modulo 12  [5] the 7-bit offsets of lanes 0..3, lane l in byte l  [6] those of lanes 4..7, lane l in byte l - 4
 * [7..9] 0  [10] crossings total  [11] hits total  [12] targets-reached total (the totals are never zeroed)  [13..15] 0.
 * Frame, back to front: black; Breakout's border; one score block per crossing of the episode, the first 19, block k at
 * x 4+4k..5+4k, y 2..3 in (236, 236, 236); the cars: lane l < L has cars on rows 12+8l..15+8l, `cars` of them, car_length
 * px long and 128 / cars apart on a wrapped track of 128 px, car k from track x (offset + k 128 / cars) mod 128; screen
 * x = track x - 22, drawn only on x 2..81, in Breakout's colour of brick row 1 + l mod 5; the walker, paddle_width x 4 px
 * at (px, py) in (200, 72, 72).  One tick (an agent step is up to action_repeat ticks: "An agent step" above, where the
 * game ends by its own condition when crossings > 0 and the episode's count >= crossings):
 *  1. steps += 1; if stun > 0 at the start of the tick: stun -= 1, the walker does not move, and rules 3 and 4 are skipped
 *     in this tick.  Else action 1: py -= ball_speed; action 2 / 3: px += / -= paddle_speed, clamped to [2, 82 - paddle_width].
 *  2. Every lane l < L whose period divides the tick counter: offset = (offset + direction speed) mod 128.  Then the tick
 *     counter grows by one, modulo 12.  (The lanes >= L keep the offset of the reset.)
 *  3. If the walker's box meets a car's box (one lane at the most: the lanes are 4 rows high and 4 apart): the reward
 *     gets hit_reward, the hits total grows, py = min(py + knock_back, 76), stun = serve_wait.  One hit per tick.
 *  4. Else if py <= 6: the reward gets cross_reward, the episode's count and the crossings total grow, the
 *     targets-reached total grows if the count now equals crossings, and the walker returns to (42 - paddle_width / 2, 76).
 *  5. terminal: crossings > 0 and count >= crossings (the target is reached: success), or steps >= max_episode_steps.
 *     With reset_on_terminal the next episode starts: episode += 1, the walker at (42 - paddle_width / 2, 76),
 *     stun = count = tick counter = steps = 0, and u = Philox4x32-10(key = seed, counter = (actor_base + b, the new
 *     episode, 0x43524F53, 0)) gives all eight offsets: word 5 = u[0] & 0x7F7F7F7F, word 6 = u[1] & 0x7F7F7F7F.  It is the
 *     game's only draw.  Without it the game goes on: the count runs past crossings, terminal stays set.
 *
 * -EINVAL without a launch: B <= 0, H1 < 2, a null or misaligned pointer the entry uses (cfg included), actor_base < 0,
 * and in the rollout entries A != 4 or a next_lar row too short for A + 1 columns. */
#define UNREAL_ARCADE_BREAKOUT 1
#define UNREAL_ARCADE_DUEL 3
#define UNREAL_ARCADE_INVADERS 5
#define UNREAL_ARCADE_CROSSING 7
#define UNREAL_ARCADE_CFG_WORDS 24
#define UNREAL_ARCADE_RECORD 16
#define UNREAL_ARCADE_SERVE_STREAM 0x41524B53
#define UNREAL_ARCADE_BOMB_STREAM 0x494E5642
#define UNREAL_ARCADE_LANE_STREAM 0x43524F53
int unreal_arcade_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward, const int* count,
                        uint8_t* frames, const int* cfg, int actor_base, int* ep_steps, int* episode, int* records,
                        void* stream);
int unreal_arcade_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                       float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                       int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                       float* episode_reward, float* score_out, int* score_valid, int reset_on_terminal, int track_score,
                       const int* cfg, int actor_base, int* ep_steps, int* episode, int* records, void* stream);
int unreal_arcade_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                               int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                               int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                               int* out_terminal, float* episode_reward, float* score_out, int* score_valid, int* active,
                               int* active_log_t, int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                               float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A, int idx_base_actor,
                               const int* cfg, int actor_base, int* ep_steps, int* episode, int* records, void* stream);
/* unreal_policy_step + unreal_arcade_rollout_step in one launch, bit-identical to the two (policy_row<4>) */
int unreal_arcade_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                      const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                      int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                      uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                      int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                      int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                      int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                      int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld, int lar_col0,
                                      int A, int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                      int* episode, int* records, void* stream);
/* Time-limit bootstrapping: the two rollout entries above with a final-observation store, as
 * unreal_maze_rollout_step_tl.  A step is a truncation when, after its last tick, steps >= max_episode_steps and the game
 * itself has not ended (Breakout: a life left and a brick left; duel: neither side at `points`; invaders: a life left and
 * an alien left; crossing: the target not reached); a step that ends the game and reaches the limit is a true end.  -EINVAL also for a null final_obs or
 * one not 16-byte aligned. */
int unreal_arcade_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                  int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                  int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                  int* out_terminal, float* episode_reward, float* score_out, int* score_valid, int* active,
                                  int* active_log_t, int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                                  float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A, int idx_base_actor,
                                  const int* cfg, int actor_base, int* ep_steps, int* episode, int* records,
                                  uint8_t* final_obs, void* stream);
int unreal_arcade_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                         const float* Wv, const float* bv, const double* u, float* pi_out, float* v_out,
                                         int* actions_out, int* pos, int* last_action, float* last_reward, int* count,
                                         uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                         int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                         int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                         int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                         int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld, int lar_col0,
                                         int A, int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                         int* episode, int* records, uint8_t* final_obs, void* stream);
/* Game mixtures: the six arcade entries above with one config block per actor.  cfg points to n_blocks
 * consecutive blocks of UNREAL_ARCADE_CFG_WORDS words (1 <= n_blocks <= UNREAL_ARCADE_MIX_MAX); global actor
 * g = actor_base + b plays block g % n_blocks for the whole run, whatever view or rank launches it.  Everything of a step
 * is the block's own: game, rules, action_repeat, return_reward, max_episode_steps and the time-limit cut of the _tl
 * forms; every actor's record is in its game's layout; the serve and bomb draws stay keyed by (seed, g, episode), so actor
 * g plays what actor g of a single-block environment of its block plays.  With n_blocks = 1 an entry computes what the
 * plain entry computes.  The arguments are the plain entry's in the same order, with n_blocks after cfg and, in the step
 * and rollout forms, done_return[B] and done_episodes[B] before stream (both or neither): when a step ends an episode
 * and track_score is set (it always is in the rollout forms), done_return[b] += the score written to score_out[b] and
 * done_episodes[b] += 1.  Per-actor accumulators without atomics; the caller zeroes them.  An actor whose block has an
 * unknown game id writes nothing; the actors of the other blocks are not affected.
 * -EINVAL without a launch: n_blocks outside 1..UNREAL_ARCADE_MIX_MAX, one of done_return / done_episodes without the
 * other, and everything the plain entry refuses. */
#define UNREAL_ARCADE_MIX_MAX 16
int unreal_arcade_mix_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                            const int* count, uint8_t* frames, const int* cfg, int n_blocks, int actor_base,
                            int* ep_steps, int* episode, int* records, void* stream);
int unreal_arcade_mix_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                           float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                           int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                           int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                           int reset_on_terminal, int track_score, const int* cfg, int n_blocks, int actor_base,
                           int* ep_steps, int* episode, int* records, float* done_return /*nullable*/,
                           int* done_episodes /*nullable*/, void* stream);
int unreal_arcade_mix_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                   int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                   int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                   int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                   int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                   int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld, int lar_col0,
                                   int A, int idx_base_actor, const int* cfg, int n_blocks, int actor_base,
                                   int* ep_steps, int* episode, int* records, float* done_return /*nullable*/,
                                   int* done_episodes /*nullable*/, void* stream);
int unreal_arcade_mix_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                          const float* Wv, const float* bv, const double* u, float* pi_out,
                                          float* v_out, int* actions_out, int* pos, int* last_action,
                                          float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                          int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                          float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                          float* score_out, int* score_valid, int* active, int* active_log_t,
                                          int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                                          float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A,
                                          int idx_base_actor, const int* cfg, int n_blocks, int actor_base,
                                          int* ep_steps, int* episode, int* records, float* done_return /*nullable*/,
                                          int* done_episodes /*nullable*/, void* stream);
int unreal_arcade_mix_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                      int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                      int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                      int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                      int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                      int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld,
                                      int lar_col0, int A, int idx_base_actor, const int* cfg, int n_blocks,
                                      int actor_base, int* ep_steps, int* episode, int* records, uint8_t* final_obs,
                                      float* done_return /*nullable*/, int* done_episodes /*nullable*/, void* stream);
int unreal_arcade_mix_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                             const float* Wv, const float* bv, const double* u, float* pi_out,
                                             float* v_out, int* actions_out, int* pos, int* last_action,
                                             float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                             int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                             float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                             float* score_out, int* score_valid, int* active, int* active_log_t,
                                             int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                                             float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A,
                                             int idx_base_actor, const int* cfg, int n_blocks, int actor_base,
                                             int* ep_steps, int* episode, int* records, uint8_t* final_obs,
                                             float* done_return /*nullable*/, int* done_episodes /*nullable*/,
                                             void* stream);
/* Self-play: the duel with both paddles driven by actors.  The six entries below take the arguments of the
 * plain arcade entries in the same order.  A launch of B actors holds B / 2 games: global actors 2 i and 2 i + 1
 * (global = actor_base + b) are seat 0 and seat 1 of game i.  cfg is ONE block of the duel (word 0 UNREAL_ARCADE_DUEL, the
 * duel's layout above); the top paddle's width is paddle_width (word 9 equals word 6; the kernels use word 6) and
 * opponent_speed (word 13) is ignored.
 * The canonical game is the duel's with two changes.  (1) The top paddle is seat 1's: its action 2 moves ox right and
 * 3 left by paddle_speed, clamped to [2, 82 - paddle_width]; the scripted follower (tick rule 2 of the duel) is not run.
 * Order within a tick: seat 0's paddle, seat 1's paddle, then the serve or the ball.  (2) Either seat serves: a waiting
 * ball is served when seat 0 or seat 1 plays 1, or by serve_wait as in the duel; the draw's key is the duel's with the
 * global index of SEAT 0 (even) as the actor word, the pair's episode and its serve_index, so both seats draw the same ball.
 * Rewards of a tick: a point for seat 0 (ty < 6) pays seat 0 win_reward and seat 1 lose_reward, a point for seat 1
 * (ty + 1 > 83) the reverse; return_reward goes to the seat whose paddle returned the ball.  An agent step is up to
 * action_repeat ticks with both actions held, none after the tick that ends the match; a seat's reward is the sum of its
 * own tick rewards.  terminal, the step limit, ep_steps and episode are the duel's and the same for both seats.
 * The mirror M of a record swaps px and ox, mine and theirs, words 10 and 11 (points won / lost totals) and words 12 and
 * 13, and sets by = 86 - by, vy = -vy; bx, vx, wait and serve_index stay.  It is applied whatever the state, so
 * M(M(g)) = g.  Word 12 is the seat's own matches-won total, word 13 (written by these entries only) the other seat's:
 * it counts the tick in which theirs reaches points, once.  records[2 i] holds the canonical record g, records[2 i + 1]
 * holds M(g), after every launch.  A seat's frame, pixel change and final observation are the duel's render of ITS OWN
 * record with opponent_width = paddle_width: every seat sees itself at the bottom in (200, 72, 72), its own score on the
 * left, and left / right mean the same on both seats.  The paddle rows 8..9 and 78..79 and the ball's rows are exact
 * images under y -> 87 - y; the field's ends are not (the canonical by ranges over 6..82, the mirrored one over 4..80,
 * so seat 1 may see the ball over the top border for a tick or two before a point): accepted.
 * One workgroup per seat (grid B).  Workgroup b reads its own record (un-mirrored if seat 1), steps the canonical game
 * with both seats' actions, takes its own reward, and renders, differences and stores its own view.  No workgroup reads a
 * word another workgroup of the launch writes: of its partner b ^ 1 it reads actions[b ^ 1], active[b ^ 1] in the plain
 * step, mask[b ^ 1] in the reset and the policy's inputs X and u.  In the plain step a pair steps only when both
 * active flags are set (else both seats idle); a pair is reset when either mask is set; in the rollout forms a seat reads
 * its own active flag, and THE CALLER keeps the two flags of a pair equal on entry (they stay equal: both seats see the
 * same terminal).  The policy forms evaluate the policy rows of b and b ^ 1 and store pi, v and the action of row b only.
 * The _tl forms keep each seat's own final observation and flag both seats 2.  reset applies the duel's reset to the
 * canonical record (ox = 42 - paddle_width / 2), then the seat's view.
 * -EINVAL without a launch: odd B, odd actor_base, and everything the plain entry refuses.  A block of another game
 * writes nothing. */
int unreal_arcade_selfplay_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                                 const int* count, uint8_t* frames, const int* cfg, int actor_base, int* ep_steps,
                                 int* episode, int* records, void* stream);
int unreal_arcade_selfplay_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                                float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                int reset_on_terminal, int track_score, const int* cfg, int actor_base, int* ep_steps,
                                int* episode, int* records, void* stream);
int unreal_arcade_selfplay_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                        int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                        int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                        int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                        int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                        int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld, int lar_col0,
                                        int A, int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                        int* episode, int* records, void* stream);
int unreal_arcade_selfplay_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                               const float* Wv, const float* bv, const double* u, float* pi_out,
                                               float* v_out, int* actions_out, int* pos, int* last_action,
                                               float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                               int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                               float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                               float* score_out, int* score_valid, int* active, int* active_log_t,
                                               int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                                               float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A,
                                               int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                               int* episode, int* records, void* stream);
int unreal_arcade_selfplay_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action,
                                           float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                           int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                                           float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                                           int* score_valid, int* active, int* active_log_t, int* n_steps,
                                           int* terminal_end, int* next_idx /*nullable*/, float* next_lar /*nullable*/,
                                           int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                           int actor_base, int* ep_steps, int* episode, int* records, uint8_t* final_obs,
                                           void* stream);
int unreal_arcade_selfplay_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                                  const float* Wv, const float* bv, const double* u, float* pi_out,
                                                  float* v_out, int* actions_out, int* pos, int* last_action,
                                                  float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                                  int* r_action, int* r_terminal, int* r_last_action,
                                                  float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                                  float* episode_reward, float* score_out, int* score_valid, int* active,
                                                  int* active_log_t, int* n_steps, int* terminal_end,
                                                  int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld,
                                                  int lar_col0, int A, int idx_base_actor, const int* cfg,
                                                  int actor_base, int* ep_steps, int* episode, int* records,
                                                  uint8_t* final_obs, void* stream);
/* Versus: self-play with ONE learner per game; the other paddle is an input.  The six entries below take the
 * arguments of the plain arcade entries in the same order, then four pointers: opp_actions [B] (read by the step forms
 * only; unused by reset), opp_frames [B x 84 * 84 * 3 bytes, 16-byte aligned], opp_last_action [B] and opp_last_reward [B].
 * A launch of B actors holds B games; B and actor_base may be odd.  Game b IS game actor_base + b of a self-play
 * environment (above): the canonical game, its rules, tick order, either-seat serve, both actions held over an agent
 * step, rewards, terminal and step limit are the self-play entries', and the serve draws are keyed by
 * 2 (actor_base + b), seat 0's global index there.  The actor is seat 0: its action is actions[b] (or the policy's draw
 * in the fused forms), seat 1's is opp_actions[b].  records[b] holds the canonical record, and the record, frame, pixel
 * change, ring slot, ep_steps, episode, rollout bookkeeping, next-step prefill, and in the _tl forms the final observation
 * and flag 2, are bit for bit what seat 0 of the self-play entries writes.
 * The opponent's side, written after the learner's: opp_frames[b] is the duel's render of M(canonical record) with
 * opponent_width = paddle_width, the frame seat 1 would see; where the step resets it is the next match's first
 * observation.  No pixel change, ring slot or final observation is kept for it.  opp_last_action[b] is the action it
 * played, opp_last_reward[b] its reward of the step; both are 0 where the step resets, as last_action[b] and
 * last_reward[b] are: the values seat 1 of the self-play entries keeps.  An idle actor (active / active_rw clear) leaves
 * all three untouched.
 * reset writes the mirrored first frame and zeroes the two words, where mask says so (mask nullable: every game).
 * One workgroup of 256 threads per game (grid B) computes the game once and forms both views; no workgroup reads a word
 * another workgroup of the launch writes.
 * -EINVAL without a launch: everything the plain entry refuses, a null or misaligned opp_frames, a null opp_last_action
 * or opp_last_reward, a null opp_actions in the step forms, and an actor_base + B beyond 2^30.  A block of another game
 * writes nothing. */
int unreal_arcade_versus_reset(int B, int H1, const int* mask, int* pos, int* last_action, float* last_reward,
                                 const int* count, uint8_t* frames, const int* cfg, int actor_base, int* ep_steps,
                                 int* episode, int* records, const int* opp_actions, uint8_t* opp_frames,
                                 int* opp_last_action, float* opp_last_reward, void* stream);
int unreal_arcade_versus_step(int B, int H1, const int* actions, const int* active, int* pos, int* last_action,
                                float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                int reset_on_terminal, int track_score, const int* cfg, int actor_base, int* ep_steps,
                                int* episode, int* records, const int* opp_actions, uint8_t* opp_frames,
                                int* opp_last_action, float* opp_last_reward, void* stream);
int unreal_arcade_versus_rollout_step(int B, int H1, const int* actions, int* pos, int* last_action, float* last_reward,
                                        int* count, uint8_t* frames, float* r_reward, int* r_action, int* r_terminal,
                                        int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                                        int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                                        int* active, int* active_log_t, int* n_steps, int* terminal_end,
                                        int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld, int lar_col0,
                                        int A, int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                        int* episode, int* records, const int* opp_actions, uint8_t* opp_frames,
                                        int* opp_last_action, float* opp_last_reward, void* stream);
int unreal_arcade_versus_policy_rollout_step(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                               const float* Wv, const float* bv, const double* u, float* pi_out,
                                               float* v_out, int* actions_out, int* pos, int* last_action,
                                               float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                               int* r_action, int* r_terminal, int* r_last_action, float* r_last_reward,
                                               float* r_pc, float* out_reward, int* out_terminal, float* episode_reward,
                                               float* score_out, int* score_valid, int* active, int* active_log_t,
                                               int* n_steps, int* terminal_end, int* next_idx /*nullable*/,
                                               float* next_lar /*nullable*/, int lar_ld, int lar_col0, int A,
                                               int idx_base_actor, const int* cfg, int actor_base, int* ep_steps,
                                               int* episode, int* records, const int* opp_actions, uint8_t* opp_frames,
                                               int* opp_last_action, float* opp_last_reward, void* stream);
int unreal_arcade_versus_rollout_step_tl(int B, int H1, const int* actions, int* pos, int* last_action,
                                           float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                                           int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc,
                                           float* out_reward, int* out_terminal, float* episode_reward, float* score_out,
                                           int* score_valid, int* active, int* active_log_t, int* n_steps,
                                           int* terminal_end, int* next_idx /*nullable*/, float* next_lar /*nullable*/,
                                           int lar_ld, int lar_col0, int A, int idx_base_actor, const int* cfg,
                                           int actor_base, int* ep_steps, int* episode, int* records, uint8_t* final_obs,
                                           const int* opp_actions, uint8_t* opp_frames, int* opp_last_action,
                                           float* opp_last_reward, void* stream);
int unreal_arcade_versus_policy_rollout_step_tl(int B, int H1, const float* X, int ldx, const float* Wp, const float* bp,
                                                  const float* Wv, const float* bv, const double* u, float* pi_out,
                                                  float* v_out, int* actions_out, int* pos, int* last_action,
                                                  float* last_reward, int* count, uint8_t* frames, float* r_reward,
                                                  int* r_action, int* r_terminal, int* r_last_action,
                                                  float* r_last_reward, float* r_pc, float* out_reward, int* out_terminal,
                                                  float* episode_reward, float* score_out, int* score_valid, int* active,
                                                  int* active_log_t, int* n_steps, int* terminal_end,
                                                  int* next_idx /*nullable*/, float* next_lar /*nullable*/, int lar_ld,
                                                  int lar_col0, int A, int idx_base_actor, const int* cfg,
                                                  int actor_base, int* ep_steps, int* episode, int* records,
                                                  uint8_t* final_obs, const int* opp_actions, uint8_t* opp_frames,
                                                  int* opp_last_action, float* opp_last_reward, void* stream);
/* host-fed environments (environment/hostfed_environment.py): environment.process + experience.add_frame of
 * every actor where active[b] != 0, for simulators on the host.  `staged` holds one uint8 frame per actor, frame_stride
 * bytes apart as in the ring (a multiple of 16 within [1200, 691200]: 20 x 20 x 3 .. 480 x 480 x 3 rounded up to 16).
 * r_pc nullable: the pixel change over pc_denom (> 0) against the stored frame, 84 x 84 only (frame_stride 21168).
 * flags: UNREAL_HOSTFED_CLIP_REWARD stores np.clip(reward, -1, 1) as the slot's reward and last reward (the environment's
 * own last_reward stays raw); UNREAL_HOSTFED_TERMINAL_OBS is the gym terminal rule: `staged` holds the terminal
 * observation of a terminal step and its pixel change is taken against it, and the next slot receives reset_staged (the
 * post-reset observation; required where reset_on_terminal, NULL without the flag) where terminal and reset_on_terminal.
 * Without it a terminal step's pixel change is 0 and `staged` holds the post-reset observation.  The three contracts:
 *   Lab     (lab_environment.py:78-119)     frame_stride 21168, r_pc, UNREAL_HOSTFED_CLIP_REWARD
 *   indoor  (indoor_environment.py:63-139)  any frame_stride (the MINOS config's height x width, main.py:196), r_pc at
 *                                           84 x 84 only (pixel control, model/model.py:416-430,554), no flags; rewards
 *                                           are divided by termination_time on the host (:111) and the objective goes
 *                                           through unreal_objective_put
 *   gym     (gym_environment.py:18-96)      frame_stride 21168 (after unreal_frame_resize), r_pc,
 *                                           UNREAL_HOSTFED_TERMINAL_OBS, reset_staged; rewards stored raw
 * active, out_reward, out_terminal nullable; episode_reward / score_out / score_valid required with track_score; staged,
 * reset_staged and frames 16-byte aligned. */
#define UNREAL_HOSTFED_CLIP_REWARD 1
#define UNREAL_HOSTFED_TERMINAL_OBS 2
int unreal_hostfed_step(int B, int H1, int frame_stride, const uint8_t* staged, const uint8_t* reset_staged,
                        const int* actions, const float* rewards, const int* terminals, const int* active,
                        int* last_action, float* last_reward, int* count, uint8_t* frames, float* r_reward, int* r_action,
                        int* r_terminal, int* r_last_action, float* r_last_reward, float* r_pc, float* out_reward,
                        int* out_terminal, float* episode_reward, float* score_out, int* score_valid,
                        int reset_on_terminal, int track_score, int flags, float pc_denom, void* stream);
/* env.reset() of every actor where mask[b] != 0 (mask nullable): the staged post-reset observation becomes the current one */
int unreal_hostfed_reset(int B, int H1, int frame_stride, const int* mask, const uint8_t* staged, int* last_action,
                         float* last_reward, const int* count, uint8_t* frames, void* stream);
/* gym / Atari raw frames (environment/gym_environment.py:18-23): src [n][Hs][Ws][3] uint8 -> dst [n][84][84][3], cv2
 * INTER_LINEAR's half-pixel rule in fp32 rounded to nearest-even (csrc/gym.hip); rows with mask[i] == 0 are skipped (mask
 * nullable). */
int unreal_frame_resize(int n, int Hs, int Ws, const uint8_t* src, const int* mask, uint8_t* dst, void* stream);
/* generic _calc_pixel_change on stored uint8 frames: out[n][400] = sum_{4x4x3}|new-old| / denom */
int unreal_pixel_change_u8(int N, const uint8_t* frames, const int* idx_new, const int* idx_old,
                           float denom, float* out, void* stream);

/* ---- counter RNG (stands in for the shared numpy RandomState of main.py:213) ----------
 * out[i] = draw number (i / row_len) * row_stride + col0 + i % row_len of Philox stream (seed, stream_id): with
 * row_len = actors of this rank, row_stride = actors of all ranks, col0 = first actor of this rank, a sharded job
 * draws exactly what one process holding every actor would (row_len = row_stride = n, col0 = 0: a plain stream). */
int unreal_philox_uniform(uint64_t seed, uint64_t stream_id, int n, int row_len, int row_stride, int col0,
                          double* out, void* stream);
int unreal_philox_randint(uint64_t seed, uint64_t stream_id, int n, int row_len, int row_stride, int col0, int high,
                          int* out, void* stream);

/* ---- replay sampling (train/experience.py:100-118, 121-153; train/trainer.py:427-434) ------------ */
int unreal_replay_sample_seq(int B, int H, int H1, int L, const int* start_draw, const int* count,
                             const int* r_terminal, int* seq_idx /*[L][B]*/, int* seq_len /*[B]*/, void* stream);
/* mode 0: this fork's buckets (reward > 0 | rest); mode 1: upstream / Lab replay (reward != 0 | reward == 0,
 * train/experience_lab_ver.py:76-80, 124-141) */
int unreal_replay_sample_rp(int B, int H, int H1, const int* coin, const double* u, const int* count,
                            const float* r_reward, int* rp_idx /*[B][3]*/, int* rp_class /*[B]*/, int mode,
                            void* stream);

/* ---- return scans (train/trainer.py:298-324, 354-372, 394-406), fp64 like the reference ----------- */
int unreal_base_returns(int B, int T, const float* rewards, const float* values, const int* n_steps,
                        const float* boot_v, const int* terminal_end, double gamma, float* R_out, float* adv_out,
                        void* stream);
/* GAE(lambda) with time-limit bootstrapping, one fp64 backward scan per actor:
 *   next_v = terminal_end[b] == 1 ? 0 : boot_v[b]   (1: a true end; 2: cut off at the step limit, boot_v = V(final
 *   observation); 0: still running, boot_v = V(s_T)); for t = n_steps[b] - 1 .. 0: delta = r_t + gamma next_v - v_t,
 *   gae = delta + gamma lambda gae, adv_t = gae, R_t = gae + v_t, next_v = v_t; rows t >= n_steps[b] are 0.
 * lambda = 1 is the n-step return of unreal_base_returns, which stays the default path's.  -EINVAL: B or T <= 0, a null
 * pointer, lambda outside [0, 1]. */
int unreal_base_returns_tl(int B, int T, const float* rewards, const float* values, const int* n_steps,
                           const float* boot_v, const int* terminal_end, double gamma, double lambda, float* R_out,
                           float* adv_out, void* stream);
/* The bootstrap pass's inputs with time-limit bootstrapping, per actor b of a group whose first actor is idx_base_actor
 * of the ring.  terminal_end[b] == 2 (and 1 <= n = n_steps[b] <= T): frame_idx[b] = final_base + idx_base_actor + b (the
 * actor's final-observation slot: final_base = actors of the whole ring * H1), c0 / h0 [b] = rows (n - 1) B + b of ws_c /
 * ws_h (the recurrent state after the last step taken), xcat[b][col0 .. col0 + A] = one-hot actions[(n - 1) B + b] |
 * rewards[(n - 1) B + b] (unclipped).  Any other actor: frame_idx[b] = (idx_base_actor + b) H1 + count[b] % H1, carried_c /
 * carried_h [b], one-hot last_action[b] | last_reward[b].  c0 null: no state is written (feed-forward); xcat null: no
 * columns.  -EINVAL: a size <= 0, H1 < 2, a negative base, a null pointer the call uses, A >= 256, ld < col0 + A + 1. */
int unreal_boot_gather(int B, int T, int H1, int idx_base_actor, int final_base, int A, const int* count,
                       const int* terminal_end, const int* n_steps, const int* last_action, const float* last_reward,
                       const int* actions, const float* rewards, const float* carried_c /*nullable*/,
                       const float* carried_h /*nullable*/, const float* ws_c /*nullable*/, const float* ws_h /*nullable*/,
                       int* frame_idx, float* c0 /*nullable*/, float* h0 /*nullable*/, float* xcat /*nullable*/, int ld,
                       int col0, void* stream);
int unreal_vr_returns(int B, int L, const int* seq_idx, const int* seq_len, const float* r_reward,
                      const int* r_terminal, const float* boot_v, double gamma, float* R_out, void* stream);
int unreal_pc_returns(int B, int L, const int* seq_idx, const int* seq_len, const float* r_pc,
                      const int* r_terminal, const float* boot_qmax, double gamma_pc, float* R_out, void* stream);

/* ---- rollout bookkeeping (train/experience.py:35-46; train/trainer.py:236-296; model.py:625-628) -- */
/* clip_reward != 0: the reward column is np.clip(r, -1, 1) (ExperienceFrame of train/experience_lab_ver.py:14,18) */
int unreal_lar_fill(int rows, int A, const int* last_action, const float* last_reward, const int* idx, float* xcat,
                    int ld, int col0, int clip_reward, void* stream);
/* objective vectors of multimodal environments (environment/indoor_environment.py:70-73,113; train/experience.py:42-44;
 * model/model.py:144,343): one [obj] fp32 row per ring slot next to the frame.  put: staged[b] -> the current slot
 * of every active actor.  fill: xcat[row][col0..col0+obj) = objective of frame idx[row] shifted by slot_offset slots
 * inside its actor's ring (-1 for the bootstrap value of train/trainer.py:300, which is fed the objective of the
 * previous frame's state). */
int unreal_objective_put(int B, int H1, int obj, const int* count, const int* active, const float* staged,
                         float* r_objective, void* stream);
int unreal_objective_fill(int rows, int obj, int H1, const float* r_objective, const int* idx, int slot_offset,
                          float* xcat, int ld, int col0, void* stream);
int unreal_gather_i32(int rows, const int* src, const int* idx, int* out, void* stream);
int unreal_rollout_advance(int B, const int* terminal_t, int* active, int* active_log_t, int* n_steps,
                           int* terminal_end, void* stream);
int unreal_seq_mask(int B, int T, const int* seq_len, int* mask, void* stream);
int unreal_reset_state(int B, const int* terminal_end, float* c, float* h, void* stream);
/* out[b] = (b0 + b) * H1 + count[b] % H1: with `count` pointing at actor b0 of a larger ring, indices into THAT ring */
int unreal_ring_cur_idx(int B, int H1, int b0, const int* count, int* out /*[B]*/, void* stream);
int unreal_seq_last_idx(int B, const int* seq_idx, const int* seq_len, int* out /*[B]*/, void* stream);
/* stats[3] (double) += {env steps, finished episodes, sum of their scores}; clears score_valid
 * (train/trainer.py:635-636 return value) */
int unreal_rollout_stats(int B, const int* n_steps, int* score_valid, const float* score_out, double* stats,
                         void* stream);

/* ---- conv encoder (model/model.py:281-289,786-787) and its gradient ------------------------------ */
int unreal_encoder_fwd(int N, const uint8_t* frames, const int* frame_idx, float frame_scale, const float* W1,
                       const float* b1, const float* W2, const float* b2, float* c1_out /*nullable [N][400][16]*/,
                       float* f2_out /*[N][2592]*/,
                       uint16_t* relu_bits /*nullable [N][81][2]: bit c of word [n][pos][h] = f2[n][pos][16h + c] > 0,
                                             i.e. bit (j % 16) of word j / 16 of row n; UNREAL_GEMM_RELU_BITS reads it */,
                       float* f2_absmax /*nullable absmax slot: max of f2_out, see unreal_absmax_f32*/,
                       float* c1_absmax /*nullable absmax slot: max of the conv1 activation (c1_out)*/,
                       const void* prepared /*nullable: block written by unreal_encoder_prepare for THESE W1, b1, W2 and
                                              frame_scale; without it every workgroup derives scales and operand
                                              fragments itself (identical results)*/,
                       void* stream);
/* The weights' share of unreal_encoder_fwd's prologue, once per weight update instead of once per workgroup and launch:
 * power-of-two scales of W1 / W2 / the conv1 planes and the fp16 hi + lo MFMA operand fragments of both convolutions ->
 * `prepared` (UNREAL_ENCODER_PREPARED_BYTES, 16-byte aligned). */
#define UNREAL_ENCODER_PREPARED_BYTES 45072
int unreal_encoder_prepare(const float* W1, const float* b1, const float* W2, float frame_scale, void* prepared,
                           long prepared_bytes, void* stream);
/* c1_absmax / d2_absmax: absmax slots covering c1_saved / d2 (the kernel keeps both as fp16 hi + lo planes with one
 * power-of-two scale per tensor, like the split GEMMs; the round-2 operand format needed none). */
int unreal_encoder_bwd(int N, const uint8_t* frames, const int* frame_idx, float frame_scale, const float* W2,
                       const float* c1_saved, const float* c1_absmax, const float* d2, const float* d2_absmax, float* dW1,
                       float* db1, float* dW2, float* db2, void* stream);

/* the conv encoder at a runtime frame size H x W, 20 <= H, W <= 480 (model/model.py:281-289,786-787 with
 * image_shape = [height, width], main.py:196; the fc widths that follow, model.py:327-333,480-484): h1 = (H - 8) / 4 + 1,
 * h2 = (h1 - 4) / 2 + 1 (w1, w2 alike).  frames [pool][H][W][3] uint8, `frame_stride` bytes apart; c1_out [N][h1][w1][16]
 * (required: conv2 reads it), f2_out [N][h2][w2][32] (the flatten of model.py:331).  fp32 operands on the fp32 matrix
 * cores (csrc/encoder_hw.hip), so no operand absmax slots; f2_absmax (nullable) receives max f2.  The backward reads d2 =
 * d(loss)/d(conv2 pre-activation), ADDS into dW1 / db1 / dW2 / db2 in a fixed order (two launches give identical bits)
 * and needs `work` of unreal_encoder_hw_work_floats(N, H, W) floats (host-only query: *out = that count). */
int unreal_encoder_hw_fwd(int N, int H, int W, const uint8_t* frames, long frame_stride, const int* frame_idx,
                          float frame_scale, const float* W1, const float* b1, const float* W2, const float* b2,
                          float* c1_out, float* f2_out, float* f2_absmax, void* stream);
int unreal_encoder_hw_bwd(int N, int H, int W, const uint8_t* frames, long frame_stride, const int* frame_idx,
                          float frame_scale, const float* W2, const float* c1_saved, const float* d2, float* work,
                          long work_floats, float* dW1, float* db1, float* dW2, float* db2, void* stream);
int unreal_encoder_hw_work_floats(int N, int H, int W, long* out, void* stream);

/* ---- dense layers: tf.matmul call sites model/model.py:314,334,423 and BasicLSTMCell 110,346-351 -- */
int unreal_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B,
                    int ldb, float* C, int ldc, const float* bias, const float* mask, int ldm, int flags,
                    int splitk, void* stream);
/* "absmax slot" = one float in device memory holding max |x| over a tensor (0-initialised by the caller; producers
 * max their outputs into it atomically).  The fp16x2 GEMMs below derive each operand's power-of-two scale from it, so
 * the slot handed to a GEMM must cover every element the GEMM reads (a larger value only costs precision).
 * unreal_absmax_f32 is the stand-alone reduction: slot = max(slot, max |x[r][c]|). */
int unreal_absmax_f32(int rows, int cols, const float* x, int ld, float* slot, void* stream);
/* C = A[M,K] * W[N,K]^T with fp32-grade error on the 16-bit matrix cores (csrc/gemm_split.hip, round 3): each operand
 * is x * 2^k = hi + lo with hi, lo fp16 (k per TENSOR, from its absmax slot), the three term pairs hh, hl, lh are
 * accumulated in fp32 on v_mfma_f32_32x32x16_f16 and un-scaled exactly.  A is fp32; W2 is the weight matrix as a
 * pre-split shadow made by unreal_split_f16x2 with the SAME w_absmax slot: plane t (0 = hi, 1 = lo) at
 * W2 + t*plane_stride, row n at + n*ldw (ldw a multiple of 8 and >= K rounded up to 32, padding zero).  c_absmax
 * (nullable): receives max |C| of what this call stores; refused (-22) together with UNREAL_GEMM_ATOMIC / splitk > 1,
 * whose epilogue adds partial tiles and never sees a finished element.  Same epilogue flags as unreal_gemm_f32.  Used
 * for the forward and dgrad GEMMs of the dense layers (tf.matmul call sites model/model.py:314,334,423). */
int unreal_gemm_f32_split_nt(int M, int N, int K, const float* A, int lda, const float* a_absmax, const uint16_t* W2,
                             int ldw, long plane_stride, const float* w_absmax, float* C, int ldc, float* c_absmax,
                             const float* bias,
                             const void* mask /* fp32 [M][ldm] (RELU_MASK: keep where > 0) or uint16 bit words [M][ldm]
                                                 (RELU_BITS: keep column j where bit j % 16 of word j / 16 is set) */,
                             int ldm, int flags, int splitk, void* stream);
/* The same product for FEW ROWS and a LONG K (the fc 2592 -> 256 of a rollout step at <= 1024 rows): the K range runs as
 * `splitk` >= 2 slabs in separate workgroups, their partial products go to `partials` (>= splitk * M * pad4(N) floats,
 * 16-byte aligned), a second launch adds them in slab order (deterministic), applies bias / ReLU (flags: 0 or 1) and
 * commits max |C| to c_absmax (nullable). */
int unreal_gemm_f32_split_nt_slabs(int M, int N, int K, const float* A, int lda, const float* a_absmax, const uint16_t* W3,
                                   int ldw, long plane_stride, const float* w_absmax, float* C, int ldc, float* c_absmax,
                                   const float* bias, int flags, int splitk, float* partials, long partial_floats,
                                   void* stream);
/* splitk > 1 needs UNREAL_GEMM_ATOMIC (K slabs added into a pre-initialised C with fp32 atomics; no ReLU / mask /
 * ACCUM then).  Measured at the per-step shapes (4096 rows): 4096x256x2592 61 -> 50 us at splitk 4, 4096x256x1024
 * slower (the atomics cost what the extra workgroups buy), so the trainer keeps splitk = 1 there. */
/* wgrad on the same scheme: C[M,N] += A[K,M]^T * B[K,N] (k = the row index of both activations), split-K with fp32
 * atomics into the caller's (pre-initialised) C.  Both operands are split while they are transposed into LDS.
 * lda, ldb multiples of 4 and A, B 16-byte aligned (else -22: use unreal_gemm_f32 transA=1).
 * colsum (nullable): colsum[n] += sum_k B[k][n], the bias gradient that belongs to this weight gradient, summed
 * from the B tiles the kernel stages anyway (saves a separate pass over B). */
/* a_absmax / b_absmax: absmax slots covering A and B (both are split as fp16 hi + lo like the NT operands; the MFMA
 * accumulators are flushed into a second fp32 set every 8 K tiles, which keeps the error under the fp32-MFMA kernel's at
 * K = 81,920). */
int unreal_gemm_f32_split_tn(int M, int N, int K, const float* A, int lda, const float* a_absmax, const float* B, int ldb,
                             const float* b_absmax, float* C, int ldc, float* colsum, int splitk, void* stream);
/* fp16x2 shadow of a weight matrix src[rows][cols]: dst[t][r][c] (transpose = 0) or dst[t][c][r] (transpose = 1),
 * dst[0] = hi, dst[1] = lo of src * 2^k, k from w_absmax (a slot that already holds max |src| over the WHOLE matrix the
 * consuming GEMM multiplies by).  dst padding is left untouched (zero it once).  Refreshed after every RMSProp step /
 * checkpoint restore. */
/* Every weight shadow of a network in one pass (round 4): `abs_descs` = n_abs records {const float* src; float* wmax; long n;
 * long block0} (contiguous matrices; block0 = first block of the record in a grid of 8192-float blocks, ascending), `split_descs`
 * = n_split records {const float* src; uint16_t* dst; const float* wmax; long rows, cols, ld_src, transpose, row_perm, ld_dst,
 * plane, tiles_x, block0} (32 x 32 tiles; the arguments of unreal_split_f16x2).  The wmax slots must be zeroed by the caller;
 * element for element the arithmetic of unreal_absmax_f32 + unreal_split_f16x2 (identical bits), in two launches instead of
 * three per matrix.  Both tables are device memory. */
int unreal_shadow_refresh_multi(const void* abs_descs, int n_abs, int abs_blocks, const void* split_descs, int n_split,
                                int split_blocks, void* stream);
int unreal_split_f16x2(int rows, int cols, const float* src, int ld_src, int transpose, int row_perm, uint16_t* dst,
                       int ld_dst, long plane_stride, const float* w_absmax, void* stream);
/* row_perm = 1 (1024 output rows only): LSTM gate interleave, output row of column n = g*256 + u of the kernel is
 * (u/16)*64 + g*16 + u%16, the layout unreal_lstm_step_fwd multiplies by. */
/* One BasicLSTMCell step (model/model.py:110,346-351; gates i,j,f,o, forget_bias 1) on the split-operand path with the
 * gate math in the GEMM epilogue.  gates [rows][1024]: out = activated gates (saved for the backward).
 *   x == NULL: gates holds the input-half pre-activations (x * Wx, hoisted over all T steps of a training sequence)
 *              on entry; W3 = gate-interleaved fp16x2 shadow of the kernel's recurrent rows [1024][256]
 *              (unreal_split_f16x2 transpose = 1, row_perm = 1) and only h_prev[rows,256] * Wh is multiplied here;
 *   x != NULL: the cell's own product [x | h_prev] @ kernel in ONE launch (a rollout step, where the input half cannot
 *              be hoisted): x[rows][Kx] (row stride ldx), W3 = gate-interleaved shadow of the WHOLE kernel,
 *              [1024][pad32(Kx) + 256]: columns [0, Kx) the input rows, zeros up to pad32(Kx), then the recurrent rows. */
/* x_absmax: slot covering x[rows][Kx] (required when x != NULL; |h_prev| < 1 is covered by the kernel itself);
 * w_absmax: the slot the shadow was made with. */
int unreal_lstm_step_fwd(int rows, const float* x, int ldx, int Kx, const float* x_absmax, const float* h_prev, int ld_hprev,
                         const uint16_t* W2, int ldw, long plane_stride, const float* w_absmax, float* gates,
                         const float* bias, const float* c_prev, float* c_out, float* h_out, int ld_h, void* stream);
/* BPTT through one recurrence step, fused: dh_rec = d_gates[rows,1024] (step t) * Wh^T on the split-operand path
 * (Wh3 = natural-layout shadow of the kernel's recurrent rows, [256][1024]), and in the same launch the gate backward
 * of step t-1 with dh = dh_above + dh_rec: dpre (d_gates of step t-1), dc_io in/out.  Same arithmetic and order as
 * unreal_gemm_f32_split_nt followed by unreal_lstm_gates_bwd (bit-identical), without materialising dh_rec. */
/* a_absmax: slot covering d_gates; dpre_absmax0 / 1 (nullable): receive max |dpre| (the next step's a_absmax, and the
 * slot of the whole sequence that the fc dgrad reads). */
int unreal_lstm_bptt_step(int rows, const float* d_gates, const float* a_absmax, const uint16_t* Wh2, int ldw,
                          long plane_stride, const float* w_absmax, const float* dh_above, float* dc_io,
                          const float* gates_act, const float* c_prev, const float* c_new, float* dpre,
                          float* dpre_absmax0, float* dpre_absmax1, void* stream);
int unreal_lstm_gates_fwd(int rows, const float* pre, const float* bias, const float* c_prev, float* gates_act,
                          float* c_out, float* h_out, int ld_h, void* stream);
int unreal_lstm_gates_bwd(int rows, const float* dh_above, const float* dh_rec, float* dc_io, const float* gates_act,
                          const float* c_prev, const float* c_new, float* dpre, float* dpre_absmax0 /*nullable*/,
                          float* dpre_absmax1 /*nullable*/, void* stream);

/* ---- heads, sampling, losses (model/model.py:358-377, 473-516, 559-576; train/trainer.py:147-148) -- */
int unreal_linear_small_fwd(int rows, int K, int NOUT, const float* X, int ldx, const float* W, const float* b,
                            float* out, int ldo, void* stream);
/* dX (nullable) (+)= dO W^T; dW[k*dw_stride_k + n*dw_stride_n] += sum_rows X[row][k] dO[row][n]
 * (strides 0,0 = the natural [K][NOUT] layout; W may be null when dX is null); db (nullable) += sum_rows dO */
int unreal_linear_small_bwd(int rows, int K, int NOUT, const float* X, int ldx, const float* dO, int ldo,
                            const float* W, float* dX, int lddx, int accumulate_dx, float* dW, int dw_stride_k,
                            int dw_stride_n, float* db, void* stream);
int unreal_softmax_sample(int rows, int A, float* logits_pi, int ld, const double* u, int* action, void* stream);
/* one rollout step of the policy in one launch: pi = softmax(X Wp + bp), v = X Wv + bv, action ~ pi (u null: arg max);
 * bit-identical to unreal_linear_small_fwd x2 + unreal_softmax_sample (K = 256 features, A in {3, 4, 6}) */
int unreal_policy_step(int rows, int A, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv,
                       const float* bv, const double* u, float* pi_out, float* v_out, int* action, void* stream);
int unreal_base_loss_grad(int rows, int A, const float* pi, int ld_pi, const float* v, const int* action,
                          const float* adv, const float* R, const int* active, float entropy_beta, float grad_scale,
                          float* dlogits, float* dv, float* losses /*[3]: policy, value, entropy*/, void* stream);
int unreal_vr_loss_grad(int rows, const float* v, const float* R, const int* mask, float grad_scale, float* dv,
                        float* loss, void* stream);
int unreal_rp_loss_grad(int rows, const float* logits, const int* cls, float grad_scale, float* prob, float* dlogits,
                        float* loss, void* stream);
/* Depth-prediction loss (csrc/depth.hip): logits [rows][ld] hold UNREAL_DEPTH_POSITIONS groups of
 * UNREAL_DEPTH_CLASSES in their first 96 columns; the label of row r, position j is r_depth[frame_idx[r] * 12 + j] (the
 * frame index the encoder read for the row; unreal_maze_depth_labels wrote the byte).  Per active row and position a
 * max-subtracted log-softmax: loss += scale * sum -log p[label]; dlogits [rows][96] = scale * (p - onehot) on active
 * rows and 0 on the others (dlogits NULL: forward only, nothing but loss and hits is written); hits[0] += positions whose
 * arg max (the lowest index on ties) is the label, hits[1] += positions counted.  scale = depth_lambda * grad_scale.
 * -EINVAL without a launch: rows <= 0, ld < 96, a null logits / r_depth / frame_idx / active / loss / hits. */
int unreal_depth_loss_grad(int rows, const float* logits, int ld, const uint8_t* r_depth, const int* frame_idx,
                           const int* active, float scale, float* dlogits /*nullable*/, float* loss, int* hits,
                           void* stream);
/* Sample reuse (csrc/ppo.hip): heads forward + clipped-surrogate (PPO) loss and gradient of `rows` re-evaluated
 * rollout rows in ONE launch, one wave per row.  pi_out [rows][A] = softmax(X Wp + bp) and v_out [rows] = X Wv + bv are
 * bit-identical to unreal_policy_step(u = NULL) (K = 256 features, ldx >= 256, A in 2..18).  With the probability clip
 * to [1e-20, 1] and its pass-through indicator `un` of unreal_base_loss_grad: pc' = clip(pi_out[a]), p_old =
 * clip(pi_old[row * ld_old + a]), rho = pc' / p_old, rc = clip(rho, 1 - clip_eps, 1 + clip_eps); per active row
 * policy loss = -min(rho adv, rc adv) - entropy_beta H(pi_out), whose unclipped term is the active one when rho adv <=
 * rc adv (a tie counts as unclipped: d/dpc' = -adv un / p_old, otherwise 0); value loss 0.25 (R - v_out)^2, dv = -0.5 (R -
 * v_out).  dlogits [rows][A] and dv [rows] are scaled by grad_scale and 0 on inactive rows (dlogits NULL: forward only,
 * neither is written).  losses[0..2] += grad_scale * (policy, value, entropy); stats_i[0] += active rows whose policy term
 * was clipped, stats_i[1] += active rows; stats_f[0] += sum (rho - 1 - ln rho), stats_f[1] += sum |rho - 1|.
 * -EINVAL without a launch: rows <= 0, a null required pointer (dv when dlogits is given), A outside 2..18, ldx < 256,
 * ld_old < A, clip_eps outside (0, 1). */
int unreal_ppo_heads_loss_grad(int rows, int A, const float* X, int ldx, const float* Wp, const float* bp, const float* Wv,
                               const float* bv, const float* pi_old, int ld_old, const int* action, const float* adv,
                               const float* R, const int* active, float clip_eps, float entropy_beta, float grad_scale,
                               float* pi_out, float* v_out, float* dlogits /*nullable*/, float* dv, float* losses /*[3]*/,
                               int* stats_i /*[2]*/, float* stats_f /*[2]*/, void* stream);
/* Count-based exploration bonus on hashed frames (csrc/explore.hip).  The code of an H x W x 3 uint8 frame in
 * the ring's byte order (y, x, channel), with cell dividing H and W, cell >= 2 and F = (H / cell) (W / cell) 3 <= 1323:
 *   S_f = sum over the cell's cell^2 pixels of min(byte, vmax),  f = ((y / cell) (W / cell) + x / cell) 3 + c
 *   level_f = S_f levels / (vmax cell^2 + 1)  (integer division),  h = sum_f level_f mult[f] mod 2^32
 *   code = (h 0x9E3779B1 mod 2^32) >> (32 - bits)
 * with levels in 2..64, vmax in 1..255, bits in 10..26: integers throughout, tests/explore_model.py is the host model.
 * unreal_explore_multipliers: mult[f] = word 0 of Philox4x32-10(key = seed, counter = (f, 0x4558504C)) | 1, f < F.
 * unreal_frame_codes: codes[r] of frame idx[r] of the pool `frames` (n_frames frames, frame_stride bytes apart: a multiple
 *   of 16 that is >= H W 3; the pointer 16-byte aligned).  One workgroup per frame: every byte is loaded once, 16 B per
 *   lane, and pooled in LDS; stride padding is loaded with the last chunk and not counted.  The optional rollout gate
 *   (active_log [rows], n_steps [B], terminal_end [B]; all three null: every row): row r = t B + b is hashed iff
 *   active_log[r] != 0 and not (terminal_end[b] != 0 and t == n_steps[b] - 1).  A gated-out row, and a row whose idx is
 *   outside [0, n_frames), reads no frame and gets code -1.  Also -EINVAL: H or W > 480, cell W 3 > 57344 (LDS).
 * unreal_count_add: table[codes[r]] += 1 (int32 atomics) for every code in [0, 2^bits); other rows are skipped.
 * unreal_count_bonus, a later launch: bonus[r] = beta / sqrtf((float)table[codes[r]]) for every such row (0 for the
 *   others); rewards_total[r] = rewards[r] + bonus[r]; r_bonus (nullable) [n_slots]: r_bonus[frame_idx[r]] = bonus[r] for
 *   every row with active_log[r] != 0 and frame_idx[r] in [0, n_slots); stats_i[0] += rows with a bonus, stats_i[1] +=
 *   those whose count is 1, stats_f[0] += sum of bonus.  beta must be finite and >= 0.
 * unreal_vr_returns_bonus: unreal_vr_returns with the reward of a step = r_reward[i] + r_bonus[i], summed in fp64.
 * Each returns -EINVAL without a launch for a size <= 0, a null required pointer or a parameter outside its range. */
int unreal_explore_multipliers(int F, uint64_t seed, uint32_t* mult, void* stream);
int unreal_frame_codes(int rows, const uint8_t* frames, long frame_stride, int n_frames, int H, int W, const int* idx,
                       int B, const int* active_log /*nullable*/, const int* n_steps /*nullable*/,
                       const int* terminal_end /*nullable*/, int cell, int levels, int vmax, int bits,
                       const uint32_t* mult, int* codes, void* stream);
int unreal_count_add(int rows, const int* codes, int* table, int bits, void* stream);
int unreal_count_bonus(int rows, const int* codes, const int* table, int bits, float beta, const float* rewards,
                       const int* active_log, const int* frame_idx, int n_slots, float* bonus, float* rewards_total,
                       float* r_bonus /*nullable*/, int* stats_i /*[2]*/, float* stats_f /*[1]*/, void* stream);
int unreal_vr_returns_bonus(int B, int L, const int* seq_idx, const int* seq_len, const float* r_reward,
                            const float* r_bonus, const int* r_terminal, const float* boot_v, double gamma, float* R_out,
                            void* stream);
int unreal_colsum(int rows, int cols, const float* X, int ld, float* out, void* stream);
int unreal_relu_mask(int rows, int cols, float* d, int ldd, const float* src, int lds, void* stream);

/* ---- pixel-control head (model/model.py:411-443, 542-557, 805-820) -------------------------------- */
/* hp [N][2592] = relu(pc_fc1); both deconvolutions + dueling combine on the fp16 matrix cores with fp16 hi + lo operands
 * (round 3): hp_absmax = absmax slot covering hp (committed by the pc_fc1 GEMM, c_absmax of unreal_gemm_f32_split_nt).
 * Bootstrap mode (qmax != NULL): max_a Q per cell.  Training mode (d_dec != NULL): loss + dL/d(pre-activation) of both
 * deconvs, and ddec_absmax (nullable slot) receives an upper bound of max |d_dec| -- the scale unreal_pc_deconv_bwd needs. */
int unreal_pc_deconv_fwd(int N, int A, const float* hp, const float* hp_absmax, const float* Wv, const float* bv,
                         const float* Wa, const float* ba, float* qmax, const int* action, const float* target,
                         const int* mask, float lambda, float grad_scale, float* d_dec, float* ddec_absmax, float* loss,
                         void* stream);
int unreal_pc_deconv_bwd(int N, int A, const float* hp, const float* hp_absmax, const float* d_dec, const float* ddec_absmax,
                         const float* Wv, const float* Wa, float* d_hp, float* dhp_absmax /*nullable absmax slot: max |d_hp|*/,
                         float* dWv, float* dbv, float* dWa, float* dba, void* stream);
/* The training pass of the head (model.py:411-443 forward, 542-557 loss, and their gradients) in ONE launch: what
 * unreal_pc_deconv_fwd (training mode) followed by unreal_pc_deconv_bwd computes, with d_dec kept on chip -- its fp16 hi + lo
 * planes take each FRAME's own power-of-two scale (max |dL/dQ| of the frame) instead of the launch's.  *loss and the four
 * parameter gradients are accumulated; d_dec is a nullable [N][400][1+A] output for inspection. */
int unreal_pc_deconv_train(int N, int A, const float* hp, const float* hp_absmax, const float* Wv, const float* bv,
                           const float* Wa, const float* ba, const int* action, const float* target, const int* mask,
                           float lambda, float grad_scale, float* loss, float* d_hp,
                           float* dhp_absmax /*nullable absmax slot: max |d_hp|*/, float* dWv, float* dbv, float* dWa,
                           float* dba, float* d_dec, void* stream);

/* ---- optimiser (train/rmsprop_applier.py:38-43, 83-93, 121) ---------------------------------------- */
int unreal_grad_norm(const float* grad, long n, float* scratch /*256 floats*/, float* norm_out, void* stream);
int unreal_rmsprop_step(float* var, float* ms, float* mom, const float* grad, long n, float lr, float decay,
                        float momentum, float eps, float clip_norm, const float* norm, void* stream);
/* Global-norm clip + Adam / AdamW (decoupled decay) over a flat fp32 buffer (csrc/adam.hip), PyTorch's
 * arithmetic in fp32:
 *   g = grad scale, scale = clip_norm min(1 / norm[0], 1 / clip_norm) when clip_norm > 0 and norm[0] > 0, else 1 (the
 *     scale of unreal_rmsprop_step; norm from unreal_grad_norm; clip_norm <= 0: no clipping, norm may be null)
 *   var <- var (1 - lr weight_decay)                 (not executed when weight_decay == 0; the kernel subtracts
 *     var lr weight_decay together with the step of the last line, so that var is rounded once per call)
 *   m <- beta1 m + (1 - beta1) g,   v <- beta2 v + (1 - beta2) g g
 *   var <- var - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * bc1 = 1 - beta1^t and bc2 = 1 - beta2^t come from the host's step count: no counter on the device, no sync.
 * -EINVAL without a launch: a null required pointer (norm only when clip_norm > 0), n <= 0, var / m / v / grad not 16-byte
 * aligned, beta1 or beta2 outside [0, 1), eps <= 0, weight_decay < 0, bc1 or bc2 outside (0, 1], a non-finite scalar. */
int unreal_adam_step(float* var, float* m, float* v, const float* grad, long n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float bc1, float bc2, float clip_norm, const float* norm,
                     void* stream);
/* Masked normalisation of a rollout's advantages (csrc/adam.hip).  Over the n rows with active[row] != 0:
 *   mean = sum adv / n,  var = sum (adv - mean)^2 / n  (population variance, two passes)
 *   adv_out = (adv - mean) / (sqrt(var) + eps) on active rows, 0 on the others; with n < 2, adv_out = adv on active rows
 *   stats[0] += mean, stats[1] += sqrt(var), stats[2] += 1  (both 0 when n = 0)
 * fp64 sums in an order that depends on `rows` alone (one workgroup): the result repeats bit for bit.  -EINVAL without a
 * launch: rows <= 0, a null pointer, eps <= 0 or non-finite, adv_out == adv. */
int unreal_adv_normalize(int rows, const float* adv, const int* active, float eps, float* adv_out, float* stats /*[3]*/,
                         void* stream);
/* Minibatched reuse epochs (csrc/minibatch.hip): the rows of the block of Bm actors that starts at actor j0 of
 * a rollout over Bg actors, compacted in ONE launch.  Source row t Bg + j0 + j -> destination row t Bm + j (t < T, j < Bm)
 * of frame_idx, actions, active (int32), adv, R (fp32) and pi (fp32, [rows][A]); with an LSTM also the `side` columns from
 * column 256 of the rows of xcat (leading dimension ld on both sides: [one-hot last action | last reward | objective], side
 * = A + 1 + objective_size; the destination's other columns are not written) and c0 / h0 [Bg][256] from actor j0 into
 * c0_out / h0_out [Bm][256], 16 bytes per lane.  A bit-exact copy; nothing past row T Bm (actor Bm) is written.
 * -EINVAL without a launch: T <= 0, Bm <= 0, j0 < 0, j0 + Bm > Bg, A outside 2..18, side < 0 or 256 + side > ld, a null
 * required pointer, some but not all of xcat, xcat_out, c0, h0, c0_out, h0_out given (feed-forward: none), a c0 / h0
 * pointer that is not 16-byte aligned. */
int unreal_minibatch_gather(int T, int Bg, int Bm, int j0, int A, const int* frame_idx, const int* actions,
                            const int* active, const float* adv, const float* R, const float* pi, int* frame_idx_out,
                            int* actions_out, int* active_out, float* adv_out, float* R_out, float* pi_out, int side, int ld,
                            const float* xcat /*nullable*/, float* xcat_out /*nullable*/, const float* c0 /*nullable*/,
                            const float* h0 /*nullable*/, float* c0_out /*nullable*/, float* h0_out /*nullable*/,
                            void* stream);

/* ---- device-to-device hand-over of 4-byte words (start_lstm_state = base_lstm_state_out, trainer.py:228-230; the
 * sampled index lists): an ordinary kernel, so the whole path can run under rocprofv3 --pmc ---------------------- */
int unreal_copy_words(long n, const void* src, void* dst, void* stream);
/* y += alpha * x: the per-call mean of the loss scalars over the G sequential updates of a grouped process() */
int unreal_axpy_f32(long n, float alpha, const float* x, float* y, void* stream);
/* buf <- the label of the kernel variant the calling thread's most recent launch used (NUL-terminated, cut to len - 1
 * characters; "" before the first launch).  Host only: no device work, no sync; `stream` is unused. */
int unreal_last_launch(char* buf, int len, void* stream);

#ifdef __cplusplus
}
#endif
#endif
