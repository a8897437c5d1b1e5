/*
 * pushworld_amd.h -- C ABI of the MI355X-native batched PushWorld step engine.
 *
 * This is the drop-in boundary for the ONE hot path of google-deepmind/pushworld
 * that this library accelerates (agent move -> push-chain closure -> collision
 * test -> goal/reward -> RGB observation).  The reference has no FFI of its own;
 * each entry point below cites the reference function it replaces (paths are
 * relative to the reference checkout).  INTEGRATION.md shows the ctypes / C++
 * stubs a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ / torch types.
 *   - every function returns 0 on success or a negative PW_E* code; no C++
 *     exception crosses the ABI; pw_last_error() returns a thread-local message.
 *   - an empty batch (batch / num_states <= 0, num_steps == 0) is a no-op that returns PW_OK without looking at
 *     the buffer pointers (an empty tensor's data pointer is NULL);
 *   - "device pointers" are caller-owned HBM buffers (e.g. tensor.data_ptr());
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *     are asynchronous on that stream; the engine never allocates per call.  Its per-environment scratch (a 16 B
 *     record per environment for the page-ordered render, 4 B for pw_step_render_delta) is allocated by
 *     pw_engine_create when PwEngineConfig::max_batch is given (or by pw_obs_alloc for its batch); with max_batch 0 the
 *     first call of a batch size allocates it, and that one call must not sit inside a graph capture.  The records are
 *     written and read by the kernels of one call, so all calls on one engine must go to ONE stream (or be
 *     event-ordered by the caller).
 *   - no entry point changes the calling thread's current HIP device: everything an engine /
 *     set / search allocates or launches lands on the device of its puzzle set, and the
 *     caller's device is restored on return.
 *   - calls on one engine must be externally serialised (like the reference
 *     objects, puzzle.py:310 / pushworld_puzzle.h:178-180, which are not
 *     re-entrant); different engines are independent.
 *
 * State layout in HBM
 *   pos        int8  [B][NP][2]   (x, y) object origins, agent first, env-major;
 *                                 NP = pw_engine_npad() in {4, 8, 16, 32}
 *   puzzle_id  int32 [B]          index into the puzzle set
 *   steps      int32 [B]          steps since the last reset (gym_env.py:201)
 *   obs        uint8|float32 [B][Hp*ppc][Wp*ppc][3] with a caller-chosen env
 *                                 stride (bytes, multiple of 16)
 */
#ifndef PUSHWORLD_AMD_H_
#define PUSHWORLD_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PW_ABI_VERSION 4

/* error codes */
#define PW_OK 0
#define PW_EINVAL (-1)     /* bad argument                                   -> ValueError    */
#define PW_EPARSE (-2)     /* malformed puzzle text (ragged rows, no agent)  -> ValueError    */
#define PW_EGOAL (-3)      /* goal without movable (puzzle.py:230-232)        -> AssertionError */
#define PW_ELIMIT (-4)     /* puzzle exceeds engine limits (W,H<=64, N<=32)   -> ValueError    */
#define PW_EDEVICE (-5)    /* HIP runtime error / no device                   -> RuntimeError  */
#define PW_ENOMEM (-6)
#define PW_EELEMENT (-7)   /* empty element name ("M1++G1"): puzzle.py:218 elem_id[0]  -> IndexError     */

/* object orderings (SURVEY trap T1) */
#define PW_ORDER_PYTHON 0  /* puzzle.py:170-257: agent, goals descending, rest in file order */
#define PW_ORDER_CPP 1     /* pushworld_puzzle.cc:262-321: agent, goals ascending, rest ascending */

/* observation element types */
#define PW_OBS_U8 0        /* puzzle.py:426-469 image bytes, zero padded                        */
#define PW_OBS_F32 1       /* env_utils.py:44-91: uint8 -> float32 / 255, zero padded            */

/* pw_step flags */
#define PW_STEP_AUTORESET 1u /* next-step autoreset: envs whose terminated|truncated flag is
                                set on entry are reset (reward 0) instead of stepped          */

#define PW_MAX_DIM 64
#define PW_MAX_OBJECTS 32
#define PW_POSITION_LIMIT 10000 /* pushworld_puzzle.h:37 */

typedef struct PwPuzzle PwPuzzle;       /* one parsed puzzle (host)                     */
typedef struct PwPuzzleSet PwPuzzleSet; /* packed bitboard/render tables (host + HBM)   */
typedef struct PwEngine PwEngine;       /* step/render configuration bound to a set     */

typedef struct PwPuzzleInfo {
  int32_t width, height;      /* puzzle.py:160-161 (includes the border walls)            */
  int32_t num_movables;       /* puzzle.py:261                                           */
  int32_t num_goals;
  int32_t num_wall_cells;
  int32_t num_agent_wall_cells; /* raw "aw" cells (without the walls, see trap T2)        */
  int32_t has_agent_walls;
  int32_t order;
} PwPuzzleInfo;

typedef struct PwEngineConfig {
  int32_t max_steps;        /* < 0: no truncation (max_steps=None, gym_env.py:223); >= 0:
                               truncated = steps >= max_steps, so 0 truncates every step   */
  int32_t pixels_per_cell;  /* puzzle.py:26, >= 1 + 2 * border_width                      */
  int32_t border_width;     /* puzzle.py:22, >= 1                                         */
  int32_t obs_dtype;        /* PW_OBS_U8 | PW_OBS_F32                                     */
  int32_t pad_cell_height;  /* observation frame in cells (env_utils.py:44-91);           */
  int32_t pad_cell_width;   /*   0 = maximum over the puzzle set (gym_env.py:80-82)       */
  int32_t max_batch;        /* > 0: the engine-owned per-environment scratch (page records of the page-ordered
                               render, dirty-row records of pw_step_render_delta) is allocated by pw_engine_create
                               for this many environments: no entry point allocates afterwards for batches up to
                               it, so the FIRST pw_step_render call may already sit inside a HIP graph capture.
                               0: allocated by the first call of a batch size (never in a steady-state loop)      */
} PwEngineConfig;

const char* pw_last_error(void);
int pw_abi_version(void);
/* number of visible HIP devices, or PW_EDEVICE */
int pw_device_count(void);

/* ------------------------------------------------------------------ puzzles (host)
 * Replaces PushWorldPuzzle.__init__ parsing, puzzle.py:130-257 /
 * pushworld_puzzle.cc:191-321.  No collision hash-tables are built: the engine
 * evaluates the reference's collision predicate on row bitboards. */
int pw_puzzle_parse(const char* text, size_t len, int order, PwPuzzle** out);
void pw_puzzle_destroy(PwPuzzle* p);
int pw_puzzle_info(const PwPuzzle* p, PwPuzzleInfo* info);
/* xy: int32 [num_movables][2] -- puzzle.py:257 initial_state */
int pw_puzzle_initial_state(const PwPuzzle* p, int32_t* xy);
/* xy: int32 [num_goals][2] -- puzzle.py:228,256 goal_state */
int pw_puzzle_goal_state(const PwPuzzle* p, int32_t* xy);
/* cells of movable `obj` relative to its origin (PushWorldObject.cells, puzzle.py:90).
 * Returns the cell count (writes at most `cap` pairs) or a negative error. */
int pw_puzzle_object_cells(const PwPuzzle* p, int obj, int32_t* xy, int cap);
int pw_puzzle_goal_cells(const PwPuzzle* p, int goal, int32_t* xy, int cap);
int pw_puzzle_wall_cells(const PwPuzzle* p, int32_t* xy, int cap);       /* puzzle.py:254 */
int pw_puzzle_agent_wall_cells(const PwPuzzle* p, int32_t* xy, int cap); /* raw "aw" cells */
/* element id ("a", "m3", ...) of movable `obj`; returns length */
int pw_puzzle_object_name(const PwPuzzle* p, int obj, char* buf, int cap);

/* --------------------------------------------------------------- puzzle set (HBM)
 * device >= 0: tables are uploaded to that HIP device.  device < 0: host-only
 * packing (inspection/tests; engines cannot be created on it). */
int pw_puzzleset_create(const PwPuzzle* const* puzzles, int n, int device, PwPuzzleSet** out);
void pw_puzzleset_destroy(PwPuzzleSet* s);
int pw_puzzleset_size(const PwPuzzleSet* s);
int pw_puzzleset_max_dims(const PwPuzzleSet* s, int* max_w, int* max_h, int* max_n);
/* packed table image (host copy), for tests */
int pw_puzzleset_blob(const PwPuzzleSet* s, const void** data, size_t* bytes);
/* Packed puzzle-set file: the compiled pool, byte for byte what sits in HBM, behind a
 * 64-byte header with format version and FNV-1a checksum.  Loading replaces parsing the puzzle
 * texts again (puzzle.py:130-311 costs the reference 3 ms .. 1.5 s per puzzle).  pw_puzzleset_load
 * validates the checksum and every table offset; PW_EPARSE for a foreign / corrupt / truncated file. */
int pw_puzzleset_save(const PwPuzzleSet* s, const char* path);
int pw_puzzleset_load(const char* path, int device, PwPuzzleSet** out);

/* ------------------------------------------------ generation / transforms / packing on the device
 * A puzzle as a *symbol grid*: one byte per cell of the file's grid (without the border walls the parser adds),
 * row-major in a square slot of slot_w x slot_w bytes, one element per cell.  The generator, the transform and the
 * packer are kernels: generate -> (transform) -> pack -> train never goes through puzzle text.  The packer writes
 * exactly the tables pw_puzzle_parse + pw_puzzleset_create produce for the same puzzle. */
#define PW_SYM_EMPTY 0x00   /* "."                                                    */
#define PW_SYM_WALL 0x01    /* "W"                                                    */
#define PW_SYM_AWALL 0x02   /* "AW"                                                   */
#define PW_SYM_AGENT 0x03   /* "A"                                                    */
#define PW_SYM_MOVABLE 0x40 /* "M<k>" = PW_SYM_MOVABLE | k, k < 48                     */
#define PW_SYM_GOAL 0x80    /* "G<k>" = PW_SYM_GOAL | k                                */

typedef struct PwGenConfig {   /* generate_level0_puzzles, generate.py:136-259 (same meaning, inclusive ranges) */
  uint64_t seed;               /* puzzle i of a seed is a pure function of (seed, i): counter-based pw_mix64 stream */
  int32_t min_size, max_size;  /* width and height of the file grid, drawn independently; max_size = slot width   */
  int32_t min_walls, max_walls;
  int32_t min_obstacles, max_obstacles;
  int32_t min_goal_objects, max_goal_objects; /* 1 .. 2 */
  int32_t complex_shapes;      /* 0: single cells ("simple"), 1: + dominoes and trominoes ("complex")            */
} PwGenConfig;

/* Puzzles first .. first + count - 1 of the stream: grids uint8 [count][max_size * max_size], dims int32 [count][2]
 * (width, height; 0 0 if no puzzle could be completed).  device >= 0: device buffers, one thread per puzzle;
 * device < 0: the same function on the host (host buffers) -- identical output. */
int pw_generate_level0(int device, const PwGenConfig* cfg, uint64_t first, int32_t count, uint8_t* grids,
                       int32_t* dims, void* stream);
/* Host only, for the distribution tests: failed[i] = how many generate_puzzle attempts of puzzle first + i raised
 * FailedToGenerateError (generate.py:236-257 retries silently) before the one that was kept; 1000 = gave up. */
int pw_generate_level0_attempts(const PwGenConfig* cfg, uint64_t first, int32_t count, int32_t* failed);
/* The 8 dihedral variants of every grid (transform.py:21-48): out uint8 [count][8][slot_w * slot_w], out_dims int32
 * [count][8][2]; variant v = 4 * flipped + clockwise quarter turns (names r0 r90 r180 r270 r0_flipped ...), the
 * top-bottom flip applied before the rotation. */
int pw_transform_grids(int device, const uint8_t* grids, const int32_t* dims, int32_t count, int32_t slot_w,
                       uint8_t* out, int32_t* out_dims, void* stream);
/* Packs `count` device-resident grids into a puzzle set on `device` (one wavefront per puzzle) -- the device-side
 * pw_puzzle_parse + pw_puzzleset_create.  Errors as the parser's: PW_EPARSE (no agent), PW_EGOAL (goal without
 * movable), PW_ELIMIT.  Synchronises `stream`. */
int pw_puzzleset_from_grids(int device, const uint8_t* grids, const int32_t* dims, int32_t count, int32_t slot_w,
                            int order, PwPuzzleSet** out, void* stream);
/* .pwp text of a HOST grid (two spaces between tokens like generate.py:133); returns the length, writes <= cap - 1 chars */
int pw_grid_to_text(const uint8_t* grid, int32_t width, int32_t height, int32_t slot_w, char* buf, int32_t cap);
/* packed header array (host copy), for tests */
int pw_puzzleset_headers(const PwPuzzleSet* s, const void** data, size_t* bytes);

/* Overlap tables (PW_OPT_STEP_TABLES) of a set as the engine builds them, for tests / inspection (host only, works on
 * device < 0 sets).  The compressed form of the reference's collision tables (puzzle.py:259-311, :522-593):
 *   pair table (i, j), R rows:  bit (rx + w_i - 1) of row (ry + h_i - 1) = movable i at (rx, ry) relative to movable j
 *                               overlaps it;  "i pushes j with displacement d" = overlap at r + d and not at r
 *   wall table j, H + 2 rows:   bit (x + 1) of row (y + 1) = movable j at (x, y) overlaps a wall (j = 0: or agent wall)
 * mode: as PW_OPT_STEP_TABLES.  dir: uint32 [count][4] = {pair_off, wall_off, R | (H + 2) << 16, 0} in 8-byte words (pair_off 0 = no tables; pair
 * table (i, j) at pair_off + (i * N + j) * R, wall table j at wall_off + j * (H + 2)).  Returns the number of words
 * (writes them when cap_words suffices). */
int64_t pw_puzzleset_overlap_tables(const PwPuzzleSet* s, int mode, uint64_t* words, int64_t cap_words, uint32_t* dir);

/* ---------------------------------------------------------------------- engine */
int pw_engine_create(const PwPuzzleSet* s, const PwEngineConfig* cfg, PwEngine** out);
void pw_engine_destroy(PwEngine* e);
int pw_engine_npad(const PwEngine* e);                 /* NP of the pos layout           */
int pw_engine_obs_shape(const PwEngine* e, int* h, int* w, int* c); /* pixels             */
int64_t pw_engine_obs_bytes(const PwEngine* e);        /* h*w*c*sizeof(elem), unpadded    */
/* name of the kernel pw_render launches for this engine (profiling aid); returns its length */
int pw_engine_render_kernel(const PwEngine* e, char* buf, int cap);
int64_t pw_engine_obs_stride(const PwEngine* e);       /* recommended env stride (16 B aligned) */

/* Engine options: kernel selection for tests / A-B runs and profiling aids.  All 0 after
 * pw_engine_create; none changes a result, only which kernel computes it. */
#define PW_OPT_STEP_KERNEL 1       /* 0 lane group per env (default), 1 wavefront per env, 2 lane per env */
#define PW_OPT_FUSED_STEP_RENDER 2 /* 1: pw_step_render is ONE launch (step inside the per-env render workgroups) */
#define PW_OPT_RENDER_KERNEL 3     /* 0 automatic, 1 per-environment LDS kernel also where a page kernel applies */
#define PW_OPT_PAGE_SLICE_ENVS 4   /* page kernels: environments per launch (0 = as many as 2^31 chunks allow) */
#define PW_OPT_SEARCH_CHUNK 5      /* pw_search_create: parents per expansion pass (0 = 2^20) */
#define PW_OPT_PROFILE_RENDER 6    /* n > 0: time the next n render launches with HIP events on their stream */
/* launch configuration of the page-ordered render kernel (same bytes, different speed; see pw_engine_tune_render) */
#define PW_OPT_PAGE_ORDER 7        /* which 4 KiB page a workgroup writes: 0 page = workgroup index, 1 the buffer in 8 >> RUN_LOG2
                                      contiguous parts, XCD k sweeping part k mod parts (RUN_LOG2 0: one eighth per XCD,
                                      1: quarters shared by two XCDs), 2 every XCD writes runs of 2^RUN_LOG2 pages */
#define PW_OPT_PAGE_RUN_LOG2 8     /* log2 of the run length of order 2 (default 6) / parts selector of order 1 */
#define PW_OPT_PAGE_LDS_PAD_KB 9   /* KiB of unused dynamic LDS per workgroup: caps the workgroups per CU, i.e. the width
                                      of the chip-wide write front (default 7 for uint8, 8 for float32 observations) */
#define PW_OPT_STEP_LDS_TABLES 10   /* the lane-group step kernel copies the puzzle's wall / shape row bitboards into LDS first
                                      and reads them from there: 0 automatic (launches of >= 4 steps on sets with more than
                                      16 movables per puzzle, where it measures ~7 % faster), 1 always, 2 never */
#define PW_OPT_TUNED_NS 11          /* read-only: nanoseconds per render launch measured for the configuration the last
                                      pw_engine_tune_render kept (0 before the first call) */
#define PW_OPT_STEP_WIDE_GROUPS 12   /* sets with 17..32 movables per puzzle (N_pad 32): 0 (default) 16 lanes per environment,
                                      two movables per lane (4 environments per wavefront); 1: 32 lanes, one movable each */
#define PW_OPT_PAGE_LOAD_ALL 13      /* ppc-3 page kernel: 1 = every page loads its static-image chunks, also the all-zero pages of
                                      the frame padding (a more even write front; a candidate of pw_engine_tune_render) */
#define PW_OPT_OBS_CHUNK_MB 14       /* pw_obs_alloc: MiB per physical chunk (0 = default, 32 MiB) */
#define PW_OPT_OBS_ACCEPT_GBS 15     /* pw_obs_alloc_tuned: a candidate on which the tuned render reaches this many GB/s is
                                      kept without looking further (default 7050 = 0.88 of the 8 TB/s peak) */
#define PW_OPT_STEP_TABLES 16         /* overlap tables for the lane-group step / expansion / search kernels (the reference's
                                      collision tables, puzzle.py:259-311, with the four actions sharing one table; one or two
                                      8-byte loads instead of a loop over object rows): 0 (default) and 1 every puzzle that fits
                                      (grids up to 62 columns, movables up to 32 wide, 256 MB in all) -- when that is every puzzle
                                      of the set the kernels carry no row loops at all; 2 none; 3 only the puzzles with a movable
                                      beyond 8 x 8 cells (kernels with both paths).  Setting it rebuilds the tables (synchronises
                                      the device) */
#define PW_OPT_STEP_TABLE_BYTES 17   /* read-only: bytes of overlap tables (and, for engines of at most 64 puzzles, push tables) in HBM */
#define PW_OPT_STEP_TABLE_PUZZLES 18 /* read-only: puzzles of the set that have overlap tables */
#define PW_OPT_STEP_NARROW_GROUPS 19 /* sets with 9..16 movables per puzzle (N_pad 16): 8 lanes per environment, two movables per lane
                                      (8 environments per wavefront) instead of 16 lanes: 0 automatic (with the table-only
                                      kernels), 1 always, 2 never.  N_pad 32 sets with the table-only kernels: 0 / 1 workgroups of
                                      32 environments run 8-lane groups unless one of them has more than 16 movables, 2 never
                                      (16-lane groups for every environment) */
#define PW_OPT_STEP_BLOCK_ORDER 20   /* lane-group step kernels: 0 workgroups take the environments in index order, 1 in reverse --
                                      for batches sorted by puzzle whose expensive puzzles (many / big movables) come last:
                                      they then start first and the cheap ones fill the tail of the launch; + 2: a contiguous eighth of
                                      the blocks per XCD (A/B runs; measured slower: profiles/r05_step_block_order.txt) */
#define PW_OPT_STEP_LANE_BATCH 21    /* state-only launches (pw_step, pw_rollout) of at least this many environments run ONE LANE per
                                      environment (the table-only formulation, 64 environments per wavefront: ~3x fewer
                                      instructions per environment than a lane group, but an eighth of the wavefronts -- it wins
                                      once the batch alone fills the chip; needs overlap tables for every puzzle of the set).
                                      0 = default (sets with up to 16 movables per puzzle: 131 072 for one step per launch, 196 608
                                      for pw_rollout; N_pad 32 sets: 327 680 and 2 097 152); a threshold no batch reaches (2^31) = never.
                                      Also the number of states from which pw_expand4 and the passes of pw_search_expand run one
                                      lane per state (default 131 072; PW_OPT_STEP_KERNEL lane forces it for every size) */
#define PW_OPT_STEP_BOARDS 22        /* sets whose puzzles ALL fit into 8 x 8 cells (grid with its border walls: the 5 x 5 Level-0
                                      families) and have at most 8 movables: state-only launches (pw_step, pw_rollout) run one lane
                                      per environment on whole-grid uint64 boards -- registers only, no table lookups.
                                      0 (default) automatic, 2 never (the lane groups) */
#define PW_OPT_STEP_BOARD_SET 23     /* read-only: 1 when the engine's set qualifies for PW_OPT_STEP_BOARDS */
#define PW_OPT_EXPAND_LDS_TABLES 24  /* pw_expand4 with one lane per state: 0 (default) the kernel that keeps the puzzle's push tables in
                                      LDS (pw_expand4_v2_kernel: 2 .. 16 movables, tables up to 112 KB, 16-byte aligned output
                                      buffers) wherever it applies, 2 never (pw_expand4_lane_kernel: tables read from HBM through L1, round 3's
                                      staging of 1 / 2 actions at a time), 3 never + all four actions staged at once and non-temporal
                                      stores (what that kernel does by itself up to 14 movables when option 0 sends a launch to it) */
#define PW_OPT_EXPAND_TILE_ORDER 25    /* pw_expand4_v2_kernel: which 64-state tiles a wavefront takes: 0 interleaved over the workgroups,
                                      1 XCD x (workgroup index mod 8) sweeps the x-th contiguous eighth of the frontier; + 2: plain
                                      instead of non-temporal stores (A/B measurements only) */
#define PW_OPT_EXPAND_PREFETCH 26      /* pw_expand4_v2_kernel: 2 (and -1, the default, for persistent workgroups) software pipeline -- a tile's successors stay staged in
                                      LDS and leave, as non-temporal whole-line stores, after the NEXT tile's parent rows have been
                                      requested; 0 a tile loads its rows at its top and stores at its end (also what runs where the
                                      pipeline's staging does not fit in 78 KB of LDS) */
#define PW_OPT_EXPAND_GROUPS_PER_CU 27 /* pw_expand4_v2_kernel: persistent workgroups per CU, 1 .. 64 (0 = automatic: with small tables and up to 8
                                      movables one workgroup per 4 tiles of 64 states -- 8 tiles at 7 and 8 movables -- whatever the
                                      frontier's size; else 8 per CU, or what is resident (at most 2) with tables beyond 32 KB) */
#define PW_OPT_STEP_MIXED_GROUPS 30 /* N_pad 8 / 16 sets with overlap tables for every puzzle: 0 (default) the lanes per environment are chosen per
                                      workgroup of 32 environments (4 / 8 / 8 with two movables per lane), 2 never (one choice per set) */
#define PW_OPT_EXPAND_WG_WAVES 29 /* pw_expand4_v2_kernel with tables so large that one workgroup fits a CU: 4 or 8 wavefronts per workgroup (0 = automatic: 8
                                    where its LDS has staging room for them) */
#define PW_OPT_SEARCH_BATCH_GROUPS_PER_CU 28 /* pw_search_batch: persistent workgroups per CU (0 = automatic) */
#define PW_OPT_STEP_QUAD16 31        /* puzzles whose grid fits 16 x 16 cells with at most 8 movables of at most 16 x 8 cells (every Level-0
                                      puzzle): workgroups whose 32 environments all play such puzzles keep every board in registers, four
                                      lanes per environment, the puzzle in ONE 576-byte record (no table, no header walk): 0 automatic
                                      (sets with overlap tables for every puzzle: the fallback for states outside the grid), 2 never */
#define PW_OPT_SEARCH_KEYS 33        /* closed set of pw_search_create (read at creation): 0 (default) fingerprint + index entries; 1 where a
                                      state packs into 63 bits (bits per coordinate x movables) and the start state overlaps no wall, a
                                      published entry is the packed state itself (a visited state is recognised without reading the
                                      stored state).  Same results and, measured, the same HBM bytes; kept for the A/B */
#define PW_OPT_EXPAND_PAIR_DIMS 34   /* pw_expand4 with the tables in LDS: 0 automatic -- byte pair tables sized PER PAIR (h_i + h_j + 2 rows of
                                      w_i + w_j + 2 bytes) where the set-wide 2 max_h + 2 by 2 max_w + 2 tables exceed 16 KB, 7 .. 16
                                      movables --, 2 never (set-wide tables, or the lane kernel where those do not fit LDS) */
#define PW_OPT_STEP_QUAD16_PUZZLES 32 /* read-only: puzzles of the set with such a record */
#define PW_OPT_MAILBOX_MODE 35       /* pw_mailbox_open (A/B runs): bits 0-1 who reads the host's word across the link -- 0 every wavefront, 1 one
                                      wavefront per workgroup, 2 one wavefront of the first workgroup, which passes it on through device
                                      memory, 3 a workgroup of its own that does nothing else and runs ahead of the stepping
                                      ones; bit 2 (+4): system-scope fences around a step instead of system-scope accesses; 11 (default, round 6) =
                                      3 pipelined: the relay wavefront reads all the slots of the ring in one trip, a stepping wavefront asks
                                      for the word two steps ahead and the next step's actions before it steps, waits ONCE after the step (for them and for the
                                      previous step's stores), writes the number of steps it has completed into a word of its own -- a publisher workgroup
                                      publishes the smallest as done: no arrive counter -- and issues this step's stores without waiting for them; bit 4 (+16): wavefront 0 keeps the per-phase clock that
                                      pw_mailbox_close_profile returns (off by default: its clock reads made wavefront 0 the slowest of the launch).  Same results (C2 round trip 38 / 10.8 /
                                      6.2 / 6.0 us: profiles/r05_mailbox.json; 11: profiles/r06_mailbox.json). */
#define PW_OPT_BIND_MIN_ENVS 36      /* pw_batch_bind: a puzzle is bound when at least this many environments of the batch play it (0 = default 48) */
#define PW_OPT_BIND_FUSED 37         /* launches of a partly bound batch: 0 (default) single steps run segments and lane groups in ONE launch (where the
                                      per-workgroup lane-group kernel applies), launches of several steps as two kernels side by side on two
                                      streams (joined by events on the caller's stream); 2 two launches one after the other on the caller's
                                      stream (A/B runs) */
#define PW_OPT_BIND_PUZZLES 38       /* read-only: puzzles of the set that can be bound (their table block fits 16 KB of LDS) */
#define PW_OPT_BIND_MISMATCHES 39    /* read-only (synchronises the device): environments that bound launches found with a puzzle id other than
                                      the one they were bound to, since the engine was created -- 0 unless the caller changed puzzle_id
                                      behind the binding's back */
#define PW_OPT_BIND_LANES 42         /* pw_batch_bind (read when binding): lanes per environment of the segments -- 0 automatic (1 up to 7 movables, 2 from 8,
                                      4 from 12, 8 from 17: a step's latency grows with the movables and a launch lasts as long as its slowest
                                      segment), 1 / 2 / 3 / 4 = at most 1 / 2 / 4 / 8 (A/B runs) */
#define PW_OPT_BIND_ROLLOUTS 43      /* launches of several steps (pw_rollout) on a bound batch: 0 (default) the segments when EVERY environment of the batch
                                      is bound, else the lane groups for all of them (measured: next to lane groups that fill the chip the
                                      segment role does not finish sooner); 1 always (segments and lane groups side by side on two streams), 2 never */
#define PW_OPT_BIND_MAX_KB 44        /* pw_batch_bind (read when binding): puzzles whose table block exceeds this many KiB of LDS stay with the lane groups
                                      (0 = default 48: every benchmark puzzle is bound; the launches carry as much LDS as the largest BOUND block) */
#define PW_OPT_BIND_SPREAD 45         /* pw_batch_bind (read when binding): environments per wavefront of the segment kernels -- 0 automatic (= 64: measured,
                                      fewer do not help: DESIGN K1g), 1 .. 5 = at most 64 / 32 / 16 / 8 / 4 (lanes per environment included; the other
                                      lanes idle); + 16 x (1 .. 5): the same for the listed environments of pw_step_mseg_kernel alone (else they
                                      follow the segments' value).  A/B runs; results do not depend on it */
#define PW_OPT_STEP_ONE_FUSED 46     /* pw_step_render_delta on a batch of ONE with a completion word (pw_engine_set_step_signal; frames of at least 64 KiB,
                                      engines other than uint8 / ppc 3): 1 (default) one launch -- workgroup 0 steps and hands positions + changed rows to
                                      the other seven through device memory, and of the changed rows only the changed COLUMNS are written --, 2 one launch writing
                                      whole rows, 0 the step kernel and the redraw as two launches (rounds 4-5).  A/B runs: same observations. */
#define PW_OPT_MAILBOX_SEG 47        /* pw_mailbox_open on a BOUND batch (pw_batch_bind) whose every environment sits in a segment, pipelined mode: 0 (default)
                                      the resident kernel runs the segments -- the puzzle's tables copied into LDS once, at the open --, 2 never (one lane
                                      per environment over the tables in memory).  Same results. */
#define PW_OPT_MAILBOX_FORM 48       /* read-only: 0 no mailbox open, 1 its kernel steps one lane per environment (whole-grid boards / tables in memory), 2 the segments
                                      of the bound batch */
#define PW_OPT_STEP_ONE_APPLIES 49    /* read-only: 1 when pw_step_render_delta on a batch of one with a completion word takes the one-launch form on this engine */
#define PW_OPT_EXPAND_FORM 50        /* read-only: the form of this engine's most recent pw_expand4 launch (0 = none yet; it records, it chooses nothing):
                                      bits 0-3 the kernel family -- 1 lane groups (pw_expand4_kernel), 2 one lane per state with the tables
                                      in memory (pw_expand4_lane_kernel), 3 pw_expand4_v2_kernel, 4 pw_expand4_v2w_kernel, 5
                                      pw_expand4_v2q_kernel --, bits 8-15 the movables N, bit 16 kPipe, bit 17 kNT (non-temporal stores),
                                      bit 18 kPD (pair tables sized per pair), bits 20-23 wavefronts per workgroup, bit 24 the tile order
                                      (PW_OPT_EXPAND_TILE_ORDER & 1), bit 25 persistent workgroups, bits 32-62 the workgroups of the
                                      grid.  Bits 16-18 and 24-25 are 0 outside families 3-5. */
#define PW_OPT_CELLS_BASE_BYTES 51   /* read-only: device bytes of the base images of the cell-grid observations (0 until the first
                                      pw_engine_cells_shape / pw_render_cells / pw_step_cells call builds them) */
#define PW_OPT_OBS_TUNE_MS 40        /* pw_obs_alloc_tuned: wall-clock budget of the candidate screen in milliseconds (0 = default 10 000): no
                                      further candidate is allocated once it is spent (the best so far is kept and tuned) -- bounds the
                                      constructor when several ranks of a node screen at the same time */
#define PW_OPT_OBS_SCREEN_MS 41      /* read-only: milliseconds the last pw_obs_alloc_tuned spent allocating, screening and releasing candidates */
/* The frame padding of a RETAINED observation buffer is written once.  A puzzle is centred in the frame, so every pixel row above and
 * below it is zero whatever the state -- on the Level-1 pool two thirds of the 4 KiB pages of a uint8 ppc-3 buffer hold nothing else.
 * With PW_OPT_OBS_PADDING_ONCE the engine keeps ONE retained observation: a buffer of pw_obs_alloc / pw_obs_alloc_tuned (at its own
 * stride, pw_engine_obs_stride rounded up to 512) whose padding was last written by a full render, by this engine, of the puzzle_id
 * buffer and batch of the current pw_batch_bind.  While that holds, pw_step_render of that batch into that buffer launches the
 * ppc-3 page kernel over the LIVE pages only -- the pages in which the full kernel stores at least one 16-byte chunk of a puzzle's
 * own pixel rows (a whole page of one environment, or the tail of one and the head of the next); it stays one timed render launch.
 *   - pw_render always writes every byte and, on such a buffer, establishes the retained observation: it is the repair path.  So do
 *     the renders of pw_engine_tune_render / pw_obs_alloc_tuned, and a pw_step_render that found nothing retained.
 *   - It ends with pw_batch_bind, pw_batch_unbind, the re-bind that pw_reset / pw_resample on the bound puzzle_id buffer do behind
 *     themselves, pw_obs_free, a render of other ids or another batch into the buffer, and with PW_OPT_PAGE_SLICE_ENVS, PW_OPT_RENDER_KERNEL
 *     or PW_OPT_FUSED_STEP_RENDER being set (none of them applies while one is set; neither does a batch that needs slices).
 *   - The contents of a retained buffer are the library's: bytes a caller writes into its padding stay there until the next pw_render.
 *   - A captured pw_step_render launch replays the form it was captured in (live pages or full), like the launches of a bound batch.
 * Buffers of the caller's own, pw_step_render_delta, the row-page kernel (ppc > 3) and the per-environment kernels are not affected.
 * The list of live pages is built on the device from the ids (pw_batch_bind reads its length back with the segment count; after a
 * re-bind in-stream the launch takes the upper bound and the surplus workgroups return); a step allocates nothing and never waits
 * for the host.  pw_engine_tune_render measures the launch configuration of the live launch in a second pass and keeps it apart from
 * PW_OPT_PAGE_* (which, set by hand afterwards, hold for both launches again). */
#define PW_OPT_OBS_PADDING_ONCE 53   /* 0 (default) every pw_step_render writes every byte; 1 as described above.  A/B runs: 2 = 1 with the grid of
                                      the full render, the workgroups of padding pages returning at once; 3 = 1 with the list of live pages
                                      (1 takes whichever the tuner measured faster, the list when it never ran) */
/* Only the CHANGED pages of a retained buffer are written (PW_OPT_OBS_CHANGED_PAGES, on top of PW_OPT_OBS_PADDING_ONCE).  A step moves the
 * agent and now and then a pushed object; only the pixel rows they leave and enter change (Level-1 pool: 29 % of the live pages).
 * The engine remembers the positions the retained buffer SHOWS (device memory laid out like pos, allocated with the live-page list; if
 * that fails the live launch stays).  Every pw_step_render / pw_render whose render goes into the retained buffer of the retained
 * (puzzle_id, batch) compares its new state with them on the device and leaves per environment the grid rows that differ (the rows a
 * moved object left and entered; all 64 when a position lies outside 0 .. 63); the launch runs over the list of live pages, and a
 * workgroup whose page holds none of those rows returns before it loads or stores anything.  A page that stays is rendered as ever.
 *   - The comparison is against what the buffer shows, not against the state before the step: pw_reset, pw_step / pw_rollout without
 *     a render, a render into another buffer, or the caller writing pos in between need no care -- the next pw_step_render repaints
 *     what they changed.  There is no precondition on pos.
 *   - The first pw_step_render after anything that establishes the retained observation anew, after pw_step_render_delta into the
 *     buffer, or after this option or PW_OPT_OBS_PADDING_ONCE was set takes the live launch (same bytes) and starts remembering.
 *   - With the option on EVERY byte of a retained buffer is the library's, not only its padding: a byte a caller writes into a live
 *     page stays until that page changes or pw_render repairs it.
 *   - A captured pw_step_render replays the form it was captured in.  The comparison runs on the device, so replays stay right while
 *     nothing else writes the buffer. */
#define PW_OPT_OBS_CHANGED_PAGES 58  /* 0 (default) the live launch; 1 as described above */
#define PW_OPT_OBS_LIVE_PAGES 54     /* read-only: length of the live-page list of the retained observation, 0 when nothing is retained (synchronises
                                      the device when the list was last rebuilt in-stream) */
#define PW_OPT_RESAMPLE_FENCE 55     /* pw_resample_weighted: 0 (default) the binary search reads the cdf alone, 1 every workgroup that draws first
                                      copies a sampled fence of the cdf into LDS.  A/B runs; same draws either way */
#define PW_OPT_STATS_LDS_PUZZLES 56  /* pw_episode_stats: largest set whose launch sums per workgroup in LDS before it adds to the block, 1 .. 1024;
                                      0 the default, 2048 never (every contributing lane adds to the block).  Same sums either way */
#define PW_OPT_STATS_GROUPS 57       /* pw_episode_stats: most workgroups of a launch (they stride over the batch); 0 (default) one per 256
                                      environments */
int pw_engine_set_option(PwEngine* e, int32_t option, int64_t value);
int64_t pw_engine_get_option(const PwEngine* e, int32_t option);
/* Only the changed pixel ROWS of a retained buffer are written: a switch on top of PW_OPT_OBS_CHANGED_PAGES (no option number; off by
 * default).  While it is on, a call that would take the changed-page launch rewrites, per environment, the 16-byte chunks that hold
 * the pixel rows of the grid rows that differ from what the buffer shows -- one wavefront per environment instead of one per page,
 * about 0.4 of the bytes.  It has no effect unless PW_OPT_OBS_CHANGED_PAGES is on and the changed form applies, and it may be set
 * between any two calls: for every legal state both forms leave the buffer equal to the positions the engine remembers.
 *   - The one state in which they differ is illegal: a movable whose y is negative (written into `pos` by a caller) but whose
 *     cells reach into the grid.  The page records skip such a movable, so pw_render and the changed-page form draw none of it;
 *     the row form rewrites every row of that environment and draws the cells that lie inside the grid.
 *   - A step no longer repairs foreign bytes elsewhere in a changed page: a byte a caller writes into a retained buffer stays until
 *     the pixel row it lies in changes.  pw_render remains the repair path.
 * pw_engine_get_obs_changed_rows returns 0 / 1, or a negative error code. */
int pw_engine_set_obs_changed_rows(PwEngine* e, int32_t on);
int32_t pw_engine_get_obs_changed_rows(const PwEngine* e);
/* Durations (milliseconds) of the render launches recorded since the last call, in launch order
 * (PW_OPT_PROFILE_RENDER).  Waits for them to finish, writes at most `cap` values, returns how many
 * were recorded and starts over. */
int pw_engine_profile_read(PwEngine* e, float* ms, int32_t cap);

/* Auto-tuning of the page-ordered render kernel's launch configuration (PW_OPT_PAGE_*): which page order and
 * occupancy is fastest depends on the physical backing of the observation buffer (measured: the same kernel
 * takes 0.545 .. 0.66 ms on buffers of identical size and alignment).  Renders (puzzle_id, pos) into `obs` with
 * every candidate configuration (a few launches each, HIP events on `stream`), keeps the fastest for this
 * engine and returns its index (0 = the default).  `obs` holds the correct observations on return; the
 * stream is synchronised.  Engines that do not use the page-ordered kernel just render.  Call once per
 * observation buffer, e.g. right after allocating it. */
int pw_engine_tune_render(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs,
                          int64_t env_stride_bytes, int32_t batch, void* stream);

/* Observation buffers owned by the library.  What the HBM-write-bound render kernel reaches on a buffer follows the
 * buffer's physical backing (two classes, 7-10 % apart, per allocation), so the library can
 * allocate the buffer itself: one reserved address range backed by physical chunks created and mapped with the HIP
 * virtual-memory API (hipMemCreate / hipMemAddressReserve / hipMemMap), batch * pw_engine_obs_stride(e) bytes,
 * zero-filled, env e at obs + e * pw_engine_obs_stride(e).  The page records of `batch` environments are allocated
 * with it, so that no later render call allocates.
 *   pw_obs_alloc        one buffer.
 *   pw_obs_alloc_tuned  allocates up to max_candidates buffers (all alive at once, so that each lands on other physical
 *                       memory), takes a quick look at each (the best of five launch configurations, three launches
 *                       each), keeps the first that is of the fast class (PW_OPT_OBS_ACCEPT_GBS; from the 16th
 *                       candidate on also one 8 % faster than the slowest seen; no further candidate once PW_OPT_OBS_TUNE_MS of wall
 *                       clock are spent) or else the fastest, RELEASES THE OTHERS TO THE DEVICE and runs
 *                       pw_engine_tune_render on the kept one.  It holds the observations of (puzzle_id, pos), the
 *                       engine its tuned launch configuration; returns the tuner's index (>= 0).  candidate_ms (host
 *                       float [max_candidates], may be NULL) receives every candidate's screened time, *tried how many
 *                       were made.
 *   (not shareable)     such a buffer is a hipMemMap range: hipIpcGetMemHandle does not apply to it.  A caller that shares
 *                       observations with other processes owns the buffer (hipMalloc) and calls pw_engine_tune_render on it.
 *   pw_obs_free         unmaps the buffer, releases its memory to the device and frees its address range (synchronises
 *                       the device first).  pw_engine_destroy frees what is left.
 * Address ranges are never handed out twice within a process (a range freed and reserved again showed stale contents
 * through views of the old one on this runtime): they are taken upwards from 32 TiB behind a watermark (O(1) state; a range
 * the runtime places below it is parked -- at most 8 per request -- and given back at process exit), ~20 000 buffers of the C3
 * size (one per candidate) in a 47-bit address space; after that the calls fail with PW_ENOMEM and the caller uses a buffer of
 * its own (VecPushWorld does, with a warning). */
int pw_obs_alloc(PwEngine* e, int32_t batch, void** obs);
int pw_obs_alloc_tuned(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t batch, int32_t max_candidates,
                       void** obs, float* candidate_ms, int32_t* tried, void* stream);
int pw_obs_free(PwEngine* e, void* obs);

/* Number of out-of-range actions (not in 0..3) the step kernels of this engine have seen since the
 * last call; reads and clears the counter, synchronises `stream`.  An asynchronous caller that never
 * looks at the 0xFF flags can poll this instead (an env flagged 0xFF is reset by the next
 * PW_STEP_AUTORESET step, where the reference raises ValueError, gym_env.py:195-196). */
int64_t pw_engine_bad_actions(PwEngine* e, void* stream);

/* Throughput counters kept ON THE DEVICE by the step kernels (the one collective of a multi-GPU job
 * sums this vector).  Every step kernel -- pw_step, pw_rollout, pw_step_render, pw_step_render_delta, whichever
 * formulation runs -- adds, per wavefront, popcount(ballot(...)) of its environments to engine-owned int64 counters
 * (64 slots a cache line apart, one atomic per wavefront and non-zero counter):
 *   out[0]  env-steps: (environment, step) pairs the kernels processed, autoreset steps and refused actions included
 *   out[1]  episodes ended: steps that returned terminated or truncated (gym_env.py:210-223)
 *   out[2]  episodes solved: steps that returned terminated (is_goal_state, puzzle.py:409-411)
 *   out[3]  actions outside 0..3 seen since the engine was created (pw_engine_bad_actions clears its own counter, not this)
 * pw_counters sums the slots (synchronises `stream`); pw_counters_reset zeroes them (asynchronous on `stream`). */
#define PW_NUM_COUNTERS 4
int pw_counters(PwEngine* e, int64_t out[PW_NUM_COUNTERS], void* stream);
int pw_counters_reset(PwEngine* e, void* stream);

/* Latency path of the single-state API (PushWorldPuzzle.get_next_state, puzzle.py:348-394; is_valid_plan :413-424;
 * render_plan :471-506): host memory in, host memory out, ONE launch and no copy command.  The state travels in the
 * kernel arguments, one wavefront computes the step(s), the result is written straight into pinned host memory mapped
 * into the device, and the call returns as soon as the kernel's completion word arrives (the calling thread polls it;
 * no stream synchronisation).  Runs on an engine-owned stream; as everything on an engine, not re-entrant.
 *   xy_in / xy_out  int8 [N][2] of puzzle `puzzle` (N = its num_movables)
 *   info            optional int32 [4]: moved-object bit mask (bit 0 = agent; 0 = nothing moved), goals achieved before,
 *                   goals achieved after, is_goal_state(after)
 * pw_plan_states replays `num_actions` actions from `xy_start` (NULL = the initial state) in one launch:
 *   states_out      int8 [num_actions + 1][N][2], state 0 = the start
 *   goal_out        optional uint8 [num_actions + 1]: is_goal_state of every state
 *   dev_states      optional DEVICE buffer int8 [num_actions + 1][NP][2] (NP = pw_engine_npad) that receives the same
 *                   states in the pos layout of pw_render, for one batched render of the whole plan
 * At most PW_PLAN_MAX_ACTIONS actions per call. */
#define PW_PLAN_MAX_ACTIONS 65536
int pw_next_state(PwEngine* e, int32_t puzzle, const int8_t* xy_in, int32_t action, int8_t* xy_out, int32_t* info);
int pw_plan_states(PwEngine* e, int32_t puzzle, const int8_t* xy_start, const uint8_t* actions, int32_t num_actions,
                   int8_t* states_out, uint8_t* goal_out, int8_t* dev_states);

/* Debug check of the preconditions of the step / render entry points: puzzle_id[i] inside the set; with `pos` != NULL
 * also every movable inside its puzzle's grid (0 <= x <= W - w, 0 <= y <= H - h) and zero padding beyond the puzzle's
 * movables.  The kernels are memory-safe without it -- a puzzle id outside the set is clamped into it, positions are
 * range-checked wherever they index a row or a table -- but then compute the step of a puzzle / state nobody meant.
 * Synchronises `stream`.  Returns the number of offending environments (0 = fine; the lowest
 * offending index goes to *first_bad when given) or a negative error. */
int64_t pw_validate_state(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t batch,
                          int32_t* first_bad, void* stream);

/* gym_env.py:150-186 reset(): pos <- initial state of puzzle_id[e], steps <- 0,
 * terminated/truncated <- 0 (when given), for envs with mask[e] != 0 (mask NULL = all). */
int pw_reset(PwEngine* e, const int32_t* puzzle_id, const uint8_t* mask, int8_t* pos,
             int32_t* steps, uint8_t* terminated, uint8_t* truncated, int32_t batch,
             void* stream);

/* Episode management on the device (the batched counterpart of
 * `self._current_puzzle = random.choice(self._puzzles)`, gym_env.py:172 / dm_env.py:172).
 * Every environment whose terminated[e] | truncated[e] flag is set (either pointer may be NULL;
 * both NULL = every environment) draws the puzzle of its next episode:
 *     episode[e] += 1
 *     r   = pw_mix64(seed, e, episode[e])          -- splitmix64 finaliser, see below
 *     idx = floor(r * n / 2^64)                     -- n = table_len, or the set size without a table
 *     puzzle_id[e] = table ? table[idx] : idx
 * `table` (device int32 [table_len], NULL = uniform over the set) holds puzzle indices, repeated to
 * weight them (e.g. the 50 % Level-0 / 50 % Level-1..4 mix of config C4).  The draw depends only on
 * (seed, e, episode[e]), not on launch geometry.  Call it before a pw_step(PW_STEP_AUTORESET): that
 * step then resets the finished environments to the initial state of their new puzzle.
 *     pw_mix64: z = seed + 0x9E3779B97F4A7C15 * (e + 1) + 0xD1B54A32D192ED03 * episode  (mod 2^64)
 *               z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *               r = z ^ z >> 31 */
uint64_t pw_mix64(uint64_t seed, uint64_t env, uint64_t episode); /* host copy of the hash above */
int pw_resample(PwEngine* e, int32_t* puzzle_id, const uint8_t* terminated, const uint8_t* truncated,
                const int32_t* table, int32_t table_len, uint64_t seed, uint32_t* episode,
                int32_t batch, void* stream);

/* The level above the single puzzle: statistics per puzzle, sampling weights made from them, and a weighted draw,
 * all on the device.  Integer arithmetic only: every result is exact and independent of launch geometry and atomic order.  The
 * three launches run on `stream`, allocate nothing, never synchronise and can be captured.  Every argument error returns PW_EINVAL
 * with the function's name and the offending argument in pw_last_error, before anything is read through a pointer.
 *
 * pw_episode_stats: called once after a step launch, on the flags that step left (with PW_STEP_AUTORESET: without it a finished
 * environment keeps its flags and would be counted by every call).  P = the size of the engine's puzzle set; `stats` is a device
 * block int64 [P][PW_EPISODE_STATS] that the caller zeroes once.  Environment i contributes when
 *     (terminated[i] | truncated[i]) != 0  and  terminated[i] != 0xFF  and  0 <= puzzle_id[i] < P
 * (a refused action is no episode end, and the episode it abandons is not counted; an id outside the set is skipped) and adds to
 * row puzzle_id[i]:  EPISODES += 1;  STEPS += steps[i];  and when terminated[i] != 0:  SOLVED += 1;  SOLVED_STEPS += steps[i].
 * batch == 0 is a no-op.  No atomic of the launch returns a value. */
#define PW_EPISODE_STATS 4   /* EPISODES, SOLVED, STEPS, SOLVED_STEPS */
#define PW_STATS_EPISODES 0
#define PW_STATS_SOLVED 1
#define PW_STATS_STEPS 2
#define PW_STATS_SOLVED_STEPS 3
int pw_episode_stats(PwEngine* e, const int32_t* puzzle_id, const int32_t* steps, const uint8_t* terminated,
                     const uint8_t* truncated, int64_t* stats, int32_t batch, void* stream);

/* pw_curriculum_update: ONE launch turns statistics into sampling weights (Q16, uint32) and their inclusive prefix sums.  Per
 * puzzle p, with n = EPISODES and s = SOLVED of stats[p] - base[p] (base NULL = zero; a negative difference counts as 0):
 *     k = max(0, bit_length(n) - 20);  n' = n >> k;  s' = min(s >> k, n');  f' = n' - s'          (unsigned 64-bit throughout)
 *     PW_CURRICULUM_UNIFORM   w = 65536
 *     PW_CURRICULUM_FAILURE   w = floor(65536 (f' + 1) / (n' + 2))                    -- unseen: 32768
 *     PW_CURRICULUM_FRONTIER  w = floor(262144 (s' + 1)(f' + 1) / (n' + 2)^2)         -- largest (65536) at a success rate of 1/2 and
 *                                                                                        unseen; the product stays below 2^61
 *     PW_CURRICULUM_GIVEN     w = given[p]                                            -- device uint32 [P]
 * then  w = max(w, floor_q16),  weights[p] = w (when given)  and  cdf[p] = w_0 + ... + w_p  (device uint64 [P]).
 * `stats` is read by FAILURE and FRONTIER only and may be NULL otherwise; `given` is read by GIVEN only. */
#define PW_CURRICULUM_UNIFORM 0
#define PW_CURRICULUM_FAILURE 1
#define PW_CURRICULUM_FRONTIER 2
#define PW_CURRICULUM_GIVEN 3
int pw_curriculum_update(PwEngine* e, int32_t mode, const int64_t* stats, const int64_t* base, const uint32_t* given,
                         uint32_t floor_q16, uint32_t* weights, uint64_t* cdf, void* stream);

/* pw_resample_weighted: pw_resample with the prefix sums of pw_curriculum_update in place of a table.  It redraws exactly the
 * environments pw_resample would (either flag non-zero; either pointer may be NULL; both NULL = every environment), on
 * pw_resample's own stream:
 *     episode[i] += 1;  r = pw_mix64(seed, i, episode[i]);  total = cdf[P - 1]
 *     total == 0:  puzzle_id[i] = mulhi64(r, P)                                  -- the uniform draw of pw_resample
 *     otherwise:   t = mulhi64(r, total);  puzzle_id[i] = the smallest p with cdf[p] > t
 * (mulhi64(a, b) = floor(a b / 2^64)), so a puzzle of weight 0 is never drawn and the draw is a pure function of
 * (seed, i, episode[i], cdf).  A bound puzzle_id buffer is re-bound behind the draw as behind pw_resample.  batch == 0 is a no-op. */
int pw_resample_weighted(PwEngine* e, int32_t* puzzle_id, const uint8_t* terminated, const uint8_t* truncated,
                         const uint64_t* cdf, uint64_t seed, uint32_t* episode, int32_t batch, void* stream);

/* The level below the single puzzle: start-state pools.  A pool holds S start states of the P puzzles of the
 * engine's set -- pool_pos int8 [S][npad][2] in the engine's state layout, a puzzle and pool_level int32 [S] (>= 0; the cost-to-go
 * for states that come from a table) -- grouped once, by the caller, by (puzzle, level):
 *     order     int32  [S]   the entries sorted by (puzzle, level), ascending entry index inside a group
 *     max_level int32  [P]   the largest level of a puzzle's entries, -1 for a puzzle without entries
 *     lvl_off   int64  [P]   where a puzzle's words start in `start`
 *     start     uint32 [start_words]   puzzle p owns max_level[p] + 2 words at lvl_off[p]; the entries of level l of puzzle p are
 *                            order[start[lvl_off[p] + l] .. start[lvl_off[p] + l + 1] - 1]  (a level without entries: empty)
 * Integer arithmetic only: every result is exact and independent of launch geometry.  The three launches run on `stream`,
 * allocate nothing, never synchronise and can be captured.  Every argument error returns PW_EINVAL with the function's name and
 * the offending argument in pw_last_error, before anything is read through a pointer.
 *
 * pw_start_pool_arm: pending[i] = (terminated[i] | truncated[i]) != 0 -- exactly the environments that the next step with
 * PW_STEP_AUTORESET will reset (the 0xFF flags of a refused action included).  Called BEFORE that step; the draw behind the step
 * takes `pending` as its mask.
 *
 * pw_start_pool_draw: one start state for every environment i < n.  mix64 is pw_mix64; the two streams are
 * PW_START_POOL_K_DRAW and PW_START_POOL_K_KEEP, distinct from PW_TABLE_K_SAMPLE / PW_TABLE_K_PLAN.
 *   1. mask != NULL and mask[i] == 0: nothing is written for i at all.
 *   2. p = puzzle_id[i].  p outside 0 .. P - 1, max_level[p] < 0 (or words of p that do not lie inside `start`):
 *      out_entry[i] = out_level[i] = -1, nothing else is written, the counter is not advanced.
 *   3. (lo, hi) = (lo_n[i], hi_n[i]) when lo_n / hi_n are given (both or neither), else band[p][0..1] when band (int32 [P][2]) is
 *      given, else the scalars lo, hi.  Then hi < 0 becomes max_level[p], then hi = max(hi, lo), then both are clamped to
 *      0 .. max_level[p].
 *   4. first = start[lvl_off[p] + lo], end = start[lvl_off[p] + hi + 1].  end <= first or end > S: the band is empty -- outs -1,
 *      the state untouched, the counter not advanced.
 *   5. ctr = ++counter[i]   (uint32, wraps).
 *   6. keep_q16 > 0 and (mix64(seed ^ PW_START_POOL_K_KEEP, i, ctr) >> 48) < keep_q16: the environment keeps the state it has
 *      (behind an autoreset: its puzzle's initial state), outs -1.  keep_q16 is in 0 .. 65536; 65536 keeps always.
 *   7. otherwise u = mulhi64(mix64(seed ^ PW_START_POOL_K_DRAW, i, ctr), end - first), entry = order[first + u]; an entry outside
 *      0 .. S - 1 (a corrupt pool) gives outs -1 and nothing else.  The npad pairs of pool_pos[entry] are copied to pos[i],
 *      steps[i] = 0, terminated[i] = truncated[i] = 0 (where the pointers are given), out_entry[i] = entry,
 *      out_level[i] = pool_level[entry].
 * npad is the engine's; n == 0 is a no-op.
 *
 * pw_start_pool_update_bands: one band int32 [P][2] = (lo, hi) per puzzle moves with the success rate of a statistics block
 * (pw_episode_stats).  Per puzzle p with max_level[p] >= 0 (the others: nothing happens), with n = EPISODES and s = SOLVED of
 * stats[p] - base[p] (a negative difference counts as 0, s is clamped to n):
 *     n < min_episodes: nothing is written and base[p] stays -- the record keeps growing.  Otherwise
 *     k = max(0, bit_length(n) - 20);  n' = n >> k;  s' = s >> k                      (as pw_curriculum_update shifts them)
 *     hi = band[p][1];  hi < 0 means max_level[p]
 *     s' * 65536 >= up_q16 * n':         hi = min(hi + step, max_level[p])
 *     else s' * 65536 < down_q16 * n':   hi = max(hi - step, min(hi_min, max_level[p]))
 *     width > 0:  lo = max(lo_min, hi - width + 1);   width == 0: lo stays
 *     band[p] = (lo, hi);  base[p][0..3] = stats[p][0..3];  delta[p] (int8 [P], may be NULL) = +1 / -1 / 0: how hi moved.
 * Refused: up_q16 < down_q16, a threshold above 65536, step < 1, min_episodes < 1, width < 0. */
#define PW_START_POOL_K_DRAW 0x8EBC6AF09C88C6E3ull
#define PW_START_POOL_K_KEEP 0x589965CC75374CC3ull
int pw_start_pool_arm(PwEngine* e, const uint8_t* terminated, const uint8_t* truncated, uint8_t* pending, int32_t n,
                      void* stream);
int pw_start_pool_draw(PwEngine* e, const int8_t* pool_pos, const int32_t* pool_level, const int32_t* order,
                       const uint32_t* start, int64_t start_words, const int64_t* lvl_off, const int32_t* max_level,
                       int32_t num_entries, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, uint64_t seed,
                       uint32_t* counter, uint32_t keep_q16, int32_t lo, int32_t hi, const int32_t* band, const int32_t* lo_n,
                       const int32_t* hi_n, int8_t* pos, int32_t* steps, uint8_t* terminated, uint8_t* truncated,
                       int32_t* out_entry, int32_t* out_level, void* stream);
int pw_start_pool_update_bands(PwEngine* e, const int32_t* max_level, const int64_t* stats, int64_t* base, int32_t* band,
                               int8_t* delta, int32_t min_episodes, uint32_t up_q16, uint32_t down_q16, int32_t step,
                               int32_t width, int32_t hi_min, int32_t lo_min, void* stream);

/* gym_env.py:188-226 step() without the observation:
 *   pos <- get_next_state(pos, action)                 puzzle.py:348-394
 *   terminated <- is_goal_state                        puzzle.py:409-411
 *   reward <- 10.0 | d(count_achieved_goals) - 0.01    gym_env.py:212-221 (float64)
 *   steps += 1; truncated <- steps >= max_steps        gym_env.py:201,223
 * reward / dgoals may be NULL.  Actions outside 0..3 leave the env untouched, set
 * terminated = truncated = 0xFF for that env and bump the engine's sticky bad-action counter
 * (pw_engine_bad_actions; the wrappers raise ValueError like gym_env.py:195-196). */
int pw_step(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos,
            int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated,
            uint8_t* truncated, int32_t batch, uint32_t flags, void* stream);

/* num_steps consecutive pw_step calls of every environment in ONE launch (state-only rollouts:
 * planner look-ahead, random-policy data, configs C2/C4).  actions is uint8 [num_steps][B],
 * step-major.  Semantics are exactly those of calling pw_step num_steps times with actions[t];
 * pos/steps/reward/dgoals/terminated/truncated receive the values after the last step.  The
 * optional histories reward_hist float64 [num_steps][B], terminated_hist / truncated_hist
 * uint8 [num_steps][B] (NULL to skip) receive every step's outputs. */
int pw_rollout(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int32_t num_steps,
               int8_t* pos, int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated,
               uint8_t* truncated, double* reward_hist, uint8_t* terminated_hist,
               uint8_t* truncated_hist, int32_t batch, uint32_t flags, void* stream);

/* BATCH BINDING: stepping at LDS-table speed for batches whose puzzle ids are known in advance (configs C2 .. C4 state-only; the
 * step half of pw_step_render).  Every pw_step / pw_rollout call takes puzzle_id afresh and walks id -> header -> table rows through
 * the caches for every push test (get_next_state, puzzle.py:348-394).  pw_batch_bind reads the ids ONCE and cuts the batch into
 * segments -- up to 256 environments of one puzzle, consecutive or not --; from then on every stepping call that passes THE SAME
 * puzzle_id pointer and batch size launches one workgroup per segment, which copies its puzzle's push tables (the reference's collision
 * tables, puzzle.py:259-311, all four actions in one nibble per offset; median 3 KB) into LDS and steps one lane per environment.
 * Environments of puzzles played by fewer than PW_OPT_BIND_MIN_ENVS environments of the batch (a C4 shard's Level-0 half: 2 per
 * puzzle), or whose tables exceed 16 KB of LDS, keep the lane groups -- in the same launch.  Same results as unbound calls, bit for bit.
 *   - ONE binding per engine; binding again replaces it; every other call (other pointers / batch sizes, pw_step_render_delta,
 *     pw_mailbox_*) works unbound as before;
 *   - the binding is a promise about the CONTENTS of puzzle_id: change them only through pw_resample or before a pw_reset on that
 *     buffer (both rebuild the list behind themselves, on their stream, without a host round trip), or bind again.  An environment
 *     whose id changed otherwise is played on the puzzle it was bound to (memory-safe; counted: PW_OPT_BIND_MISMATCHES);
 *   - pw_batch_bind synchronises `stream` (it reads the number of segments back); info (optional, int64 [6]) receives the number of
 *     segments, bound environments, bound puzzles, how many of those needed an index list (their environments not consecutive), the
 *     environments NO segment holds that launches of several steps step one lane each all the same -- 64 puzzles per wavefront, every
 *     lane with its own copy of its puzzle's block (at most 8 movables, 1 KB) in LDS -- and the bytes of such a copy's slot.
 * Measured (one C4 shard, 65 536 environments): DESIGN.md section 4 K1g. */
int pw_batch_bind(PwEngine* e, const int32_t* puzzle_id, int32_t batch, int64_t* info, void* stream);
int pw_batch_unbind(PwEngine* e);

/* RESIDENT stepping of a small state-only batch ("mailbox"): gym_env.py:188-226 for a host that needs every step's verdicts
 * before it chooses the next actions, without a kernel launch and a stream synchronisation per step.  pw_mailbox_open starts a
 * kernel that keeps the batch in registers and waits; pw_mailbox_post hands it the actions of ONE step (a word in pinned memory:
 * no launch); the kernel performs exactly what pw_step(flags) performs -- the arrays given to pw_mailbox_open receive what
 * pw_step would have written, after every step -- and leaves the step's reward / terminated / truncated in pinned host memory,
 * which pw_mailbox_wait returns once the step is complete.  Up to `ring` steps may be posted ahead of the last complete one
 * (pw_mailbox_post waits beyond that); the pointers a wait returns stay valid until `ring` more steps have been posted.
 *   - any set, batches of up to 65 536 environments (every workgroup is resident): sets whose puzzles all fit 8 x 8 cells with at
 *     most 8 movables (PW_OPT_STEP_BOARD_SET = 1: the Level-0 families of 5 x 5 puzzles) are stepped by the whole-grid boards pw_step
 *     launches for them, the others one lane per environment over their overlap tables / row bitboards (pw_step_lane_kernel's step);
 *     a batch bound with pw_batch_bind whose every environment sits in a segment (and whose segments are all resident at once) is
 *     stepped by the segments -- the puzzle's tables in LDS, copied once at the open (PW_OPT_MAILBOX_SEG / PW_OPT_MAILBOX_FORM);
 *   - puzzle_id is read once, at the open: episodes restart (PW_STEP_AUTORESET) on the same puzzle;
 *   - everything queued on other streams for the arrays must be complete before the open, and while the mailbox is open the
 *     engine's other stepping calls fail (the environments live in the resident kernel); pw_counters is current after the close
 *     (the kernel adds its sums when it has to wait for a word, every 256 steps and at its end);
 *   - `actions`: device memory, or host memory (actions_on_host != 0: copied into a pinned staging slot, read by the kernel
 *     across the link);
 *   - the kernel ends by pw_mailbox_close, or BY ITSELF after idle_ms (0 = 1 000) without a post: a resident kernel would
 *     otherwise hold every device-wide synchronisation (hipDeviceSynchronize, torch.cuda.synchronize) for ever.  pw_mailbox_post
 *     fails with PW_EDEVICE once more than idle_ms / 2 have passed since the previous post (the mailbox has expired: close it
 *     and open a new one; the arrays hold the state after the last complete step -- the Python Mailbox does exactly that by itself
 *     when no step is in flight).  Consequences for the caller: (i) a host that pauses between steps (a learner update, logging)
 *     for longer than idle_ms / 2 loses the kernel -- choose idle_ms for the longest pause of the loop; (ii) ANY device-wide
 *     synchronisation while a mailbox is open (hipDeviceSynchronize, a hipFree / hipMalloc of another allocator on the device,
 *     pw_obs_free, destroying another engine) stalls until the kernel idles out, i.e. up to idle_ms, and ends the mailbox.
 *   - one host thread at a time per mailbox (post / wait / step / run / close are not synchronised against each other).
 * Measured (C2, 4 096 environments, tools/bench_mailbox.py, profiles/r06_mailbox.json): 6.1 - 6.6 us per synchronous step against
 * 17.8 us for pw_step + a stream synchronisation; 1.95 us with 8 steps in flight (2.1e9 env-steps/s; 3.2 - 3.45 us before round 6).
 * DESIGN.md K1f. */
typedef struct PwMailbox PwMailbox;
int pw_mailbox_open(PwEngine* e, const int32_t* puzzle_id, int8_t* pos, int32_t* steps, double* reward, int8_t* dgoals,
                    uint8_t* terminated, uint8_t* truncated, int32_t batch, uint32_t flags, int32_t ring /* 0 = 8 */,
                    int32_t idle_ms /* 0 = 1000 */, PwMailbox** out);
int pw_mailbox_post(PwMailbox* m, const uint8_t* actions, int32_t actions_on_host, uint64_t* seq /* out: 1, 2, ... */);
int pw_mailbox_wait(PwMailbox* m, uint64_t seq, const double** reward, const uint8_t** terminated, const uint8_t** truncated);
/* pw_mailbox_post + pw_mailbox_wait of that step in one call; pw_mailbox_layout: where the verdicts of step `seq` are --
 * base + ((seq - 1) mod ring) * stride: reward float64 [B] at 0, terminated / truncated uint8 [B] at the two offsets. */
int pw_mailbox_step(PwMailbox* m, const uint8_t* actions, int32_t actions_on_host, uint64_t* seq);
int pw_mailbox_layout(PwMailbox* m, const uint8_t** base, int64_t* stride, int64_t* off_terminated, int64_t* off_truncated,
                      int32_t* ring);
/* num_steps posts from one uint8 [num_steps][B] array with at most `ahead` steps in flight (<= 1: every step waits for the one
 * before, the cadence of a host that chooses the next actions from a step's verdicts); returns when all are complete. */
int pw_mailbox_run(PwMailbox* m, const uint8_t* actions, int32_t num_steps, int32_t actions_on_host, int32_t ahead,
                   uint64_t* last_seq);
/* pw_mailbox_close_profile: as the close, and (profile: int64 [8], or NULL) [0] steps completed, [1] how the kernel ended (2 stop
 * word, 3 idle limit), [2..6] ticks of the device's constant clock that wavefront 0 spent waiting for the word / reading its
 * actions / stepping / storing / counting itself in (zeros unless PW_OPT_MAILBOX_MODE has bit 4 set), [7] that clock's kHz. */
int pw_mailbox_close_profile(PwMailbox* m, int64_t* profile);
int pw_mailbox_close(PwMailbox* m);

/* puzzle.py:426-469 render() + env_utils.py:44-91 padding (+ /255 for PW_OBS_F32).
 * obs: device buffer, env e at obs + e * env_stride_bytes (multiple of 16, base 16 B aligned). */
int pw_render(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs,
              int64_t env_stride_bytes, int32_t batch, void* stream);
/* pw_render_retained: the same observation, for a state that something other than this engine's pw_step_render left (DESIGN.md
 * K27: a start-state draw behind a state-only step).  Into the engine's retained buffer of the retained (puzzle_id, batch)
 * (PW_OPT_OBS_PADDING_ONCE) it writes the live pages only, and with PW_OPT_OBS_CHANGED_PAGES of those only the pages whose pixel
 * rows differ from what the buffer shows -- pw_step_render's render half, with a record pre-pass in place of the step kernel's
 * records.  Into any other buffer, or with the options off, it is pw_render.  Same bytes as pw_render either way. */
int pw_render_retained(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs,
                       int64_t env_stride_bytes, int32_t batch, void* stream);

/* pw_step followed by pw_render of the new state on the same stream (PW_OPT_FUSED_STEP_RENDER selects a
 * single launch that runs the step inside the per-environment render workgroups; slower, kept for tests). */
int pw_step_render(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos,
                   int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated,
                   uint8_t* truncated, void* obs, int64_t env_stride_bytes, int32_t batch,
                   uint32_t flags, void* stream);

/* Incremental form of pw_step_render for observation buffers that persist between steps.
 * PRECONDITION: on entry `obs` holds the observation of the state in `pos` (as left by pw_render,
 * pw_step_render or a previous pw_step_render_delta on the same buffers).  On return every output,
 * including every byte of `obs`, equals what pw_step_render produces -- but only the pixel rows swept
 * by the objects that moved are written (none for a blocked move; the whole image for environments
 * reset by PW_STEP_AUTORESET, which also covers a puzzle_id changed by pw_resample).  uint8 /
 * pixels_per_cell 3 engines; any other engine silently takes the pw_step_render path.
 * Returns PW_OK, or 1 / 2 when the launch will also write the engine's completion word (below) -- 2: the step and the redraw were ONE
 * launch (PW_OPT_STEP_ONE_FUSED) whose hand-over words carry a launch number -- a call made while its stream is being captured takes the
 * two launches (1): a graph may replay those. */
int pw_step_render_delta(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos,
                         int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated,
                         uint8_t* truncated, void* obs, int64_t env_stride_bytes, int32_t batch,
                         uint32_t flags, void* stream);

/* CELL-GRID OBSERVATIONS: a compact symbolic observation next to the RGB image, uint8 [3][Hc][Wc]
 * per environment, channel-first, Hc x Wc = the engine's frame in cells (pad_cell_height / pad_cell_width).  A puzzle of
 * H x W cells sits at row offset (Hc - H) / 2 and column offset (Wc - W) / 2 (the centring of the RGB frame at one pixel
 * per cell, env_utils.py:75-91); puzzle cell (x, y) is element [y + oy][x + ox] of every plane.
 *   plane 0  static:    0 padding, 1 floor, 2 agent wall, 3 wall (a wall is never reported as an agent wall)
 *   plane 1  occupant:  0 empty, 1 + k where movable k (index into pos[.][k], agent = 0) covers the cell at its position
 *   plane 2  goal:      0 none, 1 + k where the goal of movable k covers the cell (goal g is movable g + 1's shape at
 *                       goal g), so its codes 2 .. G + 1 equal the plane-1 code of the object that belongs there
 * Where shapes overlap (plane 1: only in invalid states) the largest k wins; cells outside the frame are dropped, so any
 * pos is memory-safe (puzzle ids are clamped to the set as in every kernel).
 * cells: device buffer, environment e at cells + e * env_stride_bytes, env_stride_bytes >= 3 Hc Wc and otherwise free
 * (no alignment is required of it or of cells: the tight stride 3 Hc Wc gives a contiguous uint8 [B][3][Hc][Wc] tensor);
 * the bytes between environments are never written.
 * The first of these three calls on an engine builds the per-puzzle base images (planes 0 and 2, 3 Hc Wc bytes per
 * puzzle rounded up to 16, PW_OPT_CELLS_BASE_BYTES): it allocates and copies synchronously, so it must not sit inside a
 * graph capture -- call pw_engine_cells_shape first.  After it, pw_render_cells / pw_step_cells allocate nothing and
 * are asynchronous on `stream` (capturable).  PW_ELIMIT when Hc Wc exceeds 65 504 cells (plane 1 is composed in LDS). */
int pw_engine_cells_shape(PwEngine* e, int* h, int* w);
/* the observation of every environment's state in pos (one launch) */
int pw_render_cells(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* cells, int64_t env_stride_bytes,
                    int32_t batch, void* stream);
/* pw_step (same arguments, same kernel choice: bound segments, lane groups, boards, autoreset, bad actions; every state
 * output bit-identical) followed on the same stream by pw_render_cells of the new state: two launches. */
int pw_step_cells(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos, int32_t* steps,
                  double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, void* cells,
                  int64_t env_stride_bytes, int32_t batch, uint32_t flags, void* stream);

/* A completion word for the single-environment adapters (gym / dm_env: batch 1, observation and state in pinned host memory):
 * `word` = 8 bytes of pinned, device-addressable host memory (NULL switches it off; the count restarts at 0).  A
 * pw_step_render_delta on a batch of ONE that redraws with the generic kernel (every engine but uint8 / pixels_per_cell 3) then
 * returns 1 instead of PW_OK and the last workgroup of its last kernel writes k -- the number of such calls since this call -- into the word after
 * everything else it wrote: the host polls the word instead of synchronising the stream (~8 us of runtime per step here). */
int pw_engine_set_step_signal(PwEngine* e, void* word);

/* For the same callers: the state arrays of their batch of one may live in DEVICE memory (a kernel that reads and writes pinned host
 * memory across the link lasts ~5 us whatever it computes) when the ONE-launch form of pw_step_render_delta applies
 * (PW_OPT_STEP_ONE_APPLIES = 1: returns 2) -- that launch then also writes a copy of what the step left into `block`, 16 + 2 * NP bytes of
 * pinned, device-addressable host memory (8-byte aligned; NULL switches it off), before the completion word:
 *   [0] reward float64 | [8] steps int32 | [12] terminated | [13] truncated | [14] dgoals int8 | [16 ...] (x, y) int8 pairs. */
int pw_engine_set_step_host_copy(PwEngine* e, void* block);

/* Planner successor expansion, best_first_search.h:76-78 calling
 * PushWorldPuzzle::getNextState (pushworld_puzzle.cc:386-460) and satisfiesGoal (:462-469)
 * for all 4 actions of F states of ONE puzzle (index `puzzle`, normally PW_ORDER_CPP).
 *   states int32 [F][N]      Position2D = x * 10000 + y   (pushworld_puzzle.h:32-37)
 *   succ   int32 [F][4][N]
 *   moved  uint32 [F][4]     bit k set <=> object k is in moved_object_indices (cc:446-457)
 *   goal   uint8 [F][4]      satisfiesGoal(successor)
 * Frontiers of >= 131 072 states run one LANE per state (engines of at most 64
 * puzzles: they carry the reference's collision tables with the four actions interleaved, 4 bits per relative offset, one
 * lookup per push test); smaller ones and other puzzles one lane group per state.  Same results either way; the buffers need
 * no particular alignment (16-byte aligned ones leave in wider stores).  PW_OPT_STEP_LANE_BATCH moves the threshold. */
int pw_expand4(PwEngine* e, int32_t puzzle, const int32_t* states, int32_t* succ,
               uint32_t* moved, uint8_t* goal, int32_t num_states, void* stream);

/* ---------------------------------------------------------- planner frontier services
 * Breadth-first exploration of ONE puzzle with the closed set on the device.  The reference
 * planner pops one node, calls getNextState x4 and looks each successor up in a
 * std::unordered_set<State> (best_first_search.h:72-93); here every call expands a whole layer:
 * pw_expand4 semantics for the successors, an open-addressing visited table in HBM, and the new
 * states appended to a store with (parent, action) links.  State numbering is deterministic and
 * equals the one of a sequential FIFO search trying the actions in the order 0..3 (state 0 = start).
 * All device memory is allocated by pw_search_create (about max_states * (2N + 40) bytes + scratch: the
 * visited table is 16 .. 32 bytes per state -- 8-byte slots of (fingerprint, entry) at a load factor below one half). */
/* Novelty tables: NoveltyHeuristic::estimate_cost_to_goal (cpp/src/heuristics/novelty.cc:30-77) for a
 * whole array of states.  novelty[k] is what the reference returns for state k when the states are fed
 * to it one after the other in index order, this call after all earlier calls: 1 = a moved object is at
 * a position it never had, 2 = a (moved object, other object) pair of positions is new, 3 = neither.
 *   states  device int32 [count][state_size] Position2D, inside the width x height grid
 *   moved   device uint32 [count], bit i = object i is in moved_object_indices (pw_expand4's `moved`)
 * Memory: state_size * (state_size - 1) / 2 * (width * height)^2 * 4 bytes for the pair table. */
typedef struct PwNovelty PwNovelty;
int pw_novelty_create(int device, int state_size, int width, int height, PwNovelty** out);
void pw_novelty_destroy(PwNovelty* n);
int pw_novelty_reset(PwNovelty* n, void* stream);
int pw_novelty_eval(PwNovelty* n, const int32_t* states, const uint32_t* moved, uint8_t* novelty,
                    int32_t count, void* stream);

typedef struct PwSearch PwSearch;
/* novelty_width 0: breadth-first search.  1 or 2: width-limited search IW(k) (Lipovetzky & Geffner) on
 * the reference's novelty definition: every new state gets its novelty (tables updated in discovery
 * order, the start state with all objects moved, best_first_search.h:58-67); states whose novelty exceeds
 * the width stay in the closed set but are not expanded. */
int pw_search_create(PwEngine* e, int32_t puzzle, int64_t max_states, int32_t novelty_width, PwSearch** out);
void pw_search_destroy(PwSearch* s);
/* start: host int32 [N] Position2D (x * 10000 + y), NULL = the puzzle's initial state */
int pw_search_begin(PwSearch* s, const int32_t* start, void* stream);
/* Expands the newest layer and synchronises the stream.
 *   info[0] depth of the new layer   info[1] states in it (0 = search space exhausted)
 *   info[2] states in the store      info[3] lowest index of a goal state found so far, or -1
 * PW_ELIMIT when the store is full (the new layer is then incomplete). */
int pw_search_expand(PwSearch* s, int64_t info[4], void* stream);
/* dst: device int32 [count][N] Position2D of states first .. first + count - 1 */
int pw_search_read_states(PwSearch* s, int64_t first, int64_t count, int32_t* dst, void* stream);
/* device int32 [count] parent indices (-1 for the start) and uint8 [count] actions; either may be NULL */
int pw_search_read_links(PwSearch* s, int64_t first, int64_t count, int32_t* parent, uint8_t* action,
                         void* stream);
/* device uint8 [count]: 1 = state was cut by the novelty width (never expanded), 0 otherwise */
int pw_search_read_flags(PwSearch* s, int64_t first, int64_t count, uint8_t* pruned, void* stream);
/* actions (host buffer) from the start to state `index`; returns the plan length (if > cap nothing
 * is written: call again with a larger buffer) or a negative error. */
int pw_search_plan(PwSearch* s, int64_t index, uint8_t* actions, int32_t cap, void* stream);

/* Exact cost-to-go table over an EXHAUSTED breadth-first search (novelty_width 0, the last pw_search_expand reported 0 new
 * states, the store did not overflow; anything else: PW_EINVAL naming the condition).  One row per state of the store:
 *   succ  int32 [total][4]  store index of the successor under L, R, U, D; the state's own index where the action moves nothing
 *   cost  uint16 [total]    length of a shortest action sequence to a goal state: 0 at every goal state (whatever lies beyond
 *                           it), 0xFFFF where no goal state can be reached (a dead end: PushWorld is irreversible)
 *   acts  uint8 [total]     bit a (0..3): action a is optimal -- succ[i][a] != i and cost[succ[i][a]] == cost[i] - 1 (none at goal
 *                           states and dead ends); bit 4 + a: action a is safe -- cost[succ[i][a]] is finite (an action that
 *                           moves nothing out of a solvable state is safe)
 * pw_search_solve is synchronous: a successor pass (the store expanded again, every successor looked up in the closed set --
 * exactly, with either entry form of PW_OPT_SEARCH_KEYS), then level-synchronous backward sweeps from the goal states.
 *   info[0] states   info[1] goal states   info[2] dead ends   info[3] largest finite cost
 * PW_ELIMIT when a finite cost reaches 65 535; PW_EDEVICE when a successor is missing from the closed set (an internal error).
 * Memory: 19 bytes per state of the store as it stands (16 succ + 2 cost + 1 acts; the sweeps work in place), 256 KB of
 * counters, and with exact keys 4 bytes per slot of the visited table (which state sits in which slot).  pw_search_begin and
 * pw_search_destroy discard the table. */
int pw_search_solve(PwSearch* s, int64_t info[4], void* stream);
/* The last pw_search_solve: device milliseconds of [0] the successor pass, [1] the backward sweeps, [2] the action bits
 * (-1: not measured); [3] successor passes, [4] how many of them ran the one-lane-per-parent expansion kernel. */
int pw_search_solve_stats(PwSearch* s, double stats[5]);
/* rows first .. first + count - 1 into device buffers (any of them may be NULL); asynchronous on `stream` */
int pw_search_table_read(PwSearch* s, int64_t first, int64_t count, int32_t* succ, uint16_t* cost, uint8_t* acts, void* stream);
/* Live states -> table rows: ONE launch, asynchronous on `stream`, no allocation, no synchronisation (capturable).
 *   puzzle_id  device int32 [n], or NULL: every item is of the table's puzzle
 *   pos        device int8 [n][npad][2], the engine's state layout (pw_plan_batch_run_states'); npad 4 / 8 / 16 / 32
 *   mask       device uint8 [n] or NULL: 0 skips an item
 * For every item of the table's puzzle that is not masked out (any output may be NULL):
 *   index[i]   the store index, -1 when the state is not in the table (not reachable from the search's start, or a
 *              coordinate outside the grid)
 *   cost[i]    the cost, -1 for a dead end, -2 when the state is not in the table
 *   acts[i]    the action bits, 0 when the state is not in the table
 * Items of other puzzles and masked items are LEFT UNTOUCHED: several tables fill one set of outputs for a mixed batch.
 * PW_EINVAL before any launch, pw_last_error naming the function: null handle, n < 1, null pos, npad not 4 / 8 / 16 / 32 or
 * smaller than the puzzle's number of movables, no solved table. */
int pw_search_table_query(PwSearch* s, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                          int32_t n, int32_t* index, int32_t* cost, uint8_t* acts, void* stream);

/* Batched search of SMALL puzzles: ONE launch decides solvability for `n` puzzles of the engine's set (the filter of
 * generate.py:262-297 over a generated set; best_first_search.h:45-98 with a FIFO frontier).  Persistent workgroups take
 * puzzles off a device counter and run the whole breadth-first loop inside the kernel -- closed set in LDS (4 096 states)
 * that moves to the workgroup's HBM slab when a layer could outgrow it, no launch per layer, no host readback.
 *   puzzles     device int32 [n] set indices, NULL = 0 .. n - 1
 *   verdict     device uint8 [n]: 1 solved, 0 unsolvable (reachable space exhausted), 2 unknown (more than
 *               max_states_each states), 3 not searched -- the kernel handles grids up to 16 x 16 (with their border) and up
 *               to 8 movables (every Level-0 recipe) of puzzles with overlap tables; search the others with pw_search_create
 *   plan_len    device int32 [n]: length of a shortest plan (depth of the first goal state), -1 unless solved
 *   num_states  optional device int32 [n]: states in the closed set when the search ended
 *   plans       optional device uint8 [n][plan_cap]: the actions of A shortest plan of every solved puzzle whose plan fits
 *               plan_cap (the layers are not numbered in FIFO order here: pw_search_plan's plan is the first in action order,
 *               this one is any of the same length); costs 4 more bytes per state of slab
 * novelty_width must be 0 (breadth-first; the width-limited IW(k) is pw_search_create's).  The slabs (8 bytes per state of
 * store + the tables, per persistent workgroup) are engine-owned, allocated on first use / growth (synchronises `stream`
 * then) and kept.  Asynchronous on `stream` otherwise. */
int pw_search_batch(PwEngine* e, const int32_t* puzzles, int32_t n, int64_t max_states_each, int32_t novelty_width,
                    uint8_t* verdict, int32_t* plan_len, int32_t* num_states, uint8_t* plans, int32_t plan_cap, void* stream);

/* Exact cost-to-go tables (pw_search_solve's rows: succ, cost, acts, same definitions) of MANY small puzzles in ONE launch,
 * in the form of pw_search_batch: persistent workgroups take puzzles off a device counter and do the exhaustive
 * breadth-first search, the successor pass, the backward sweeps (a barrier each, not a launch each) and the action bits of
 * a puzzle inside the kernel.  Same limits as pw_search_batch (16 x 16 cells with the border, 8 movables, overlap tables).
 *
 * pw_solve_batch_create: rows_cap >= 0 rows of pool for the tables of all items together (0: summaries only).
 * pw_solve_batch_run: `puzzles` device int32 [n] set indices or NULL = 0 .. n - 1, n >= 1; asynchronous on `stream` except
 *   when the engine's slabs or the handle's per-item arrays have to grow (first call, larger n or max_states_each).
 * Per item, in device arrays owned by the handle (pw_solve_batch_results; valid until the next run or the destroy):
 *   status   uint8      0 table built and stored   2 more than max_states_each states   3 not searched (beyond the limits)
 *                       4 built, but the row pool was full: the summary is valid, the rows are not stored
 *                       5 a finite cost reached 65 535   6 a successor was missing from the exhausted closed set (internal)
 *   summary  int32 [5]  states, goal states, dead ends, largest finite cost, cost of the start state (-1: a dead end);
 *                       valid for status 0 and 4 (else: states found so far, then 0 0 0 -1)
 *   row_off  int64      first row of the item's table in the pool, -1 when it is not stored
 * A workgroup reserves the rows of a finished table with one atomicAdd, so WHICH offset an item gets -- and the numbering
 * of the states inside one breadth-first layer, hence which row a state has -- depends on the schedule and may differ from
 * run to run.  Everything else does not: row 0 is the start state, rows are found by state (key / pw_solve_batch_query),
 * succ holds row numbers within the item's table.  An item that did not fit leaves its reservation unused.
 * pw_solve_batch_totals (synchronises `stream`): [0] the rows a pool needs to store every built table of the run (size a
 *   second handle with it), [1] lookup slots in use, [2] missing successors (0).
 * pw_solve_batch_read: rows first .. first + count - 1 of a stored item into device buffers (any may be NULL):
 *   key   uint64     the state: movable j at bits 8 j (x in the low nibble, y in the high one), zeros beyond the puzzle's N
 *   succ  int32 [4]  cost  uint16  acts  uint8   as pw_search_table_read
 *   The first read after a run fetches the item offsets (synchronises `stream` once); asynchronous afterwards.
 * pw_solve_batch_query: live states of a MIXED batch -> rows, ONE launch, no allocation, no synchronisation (capturable).
 *   puzzle_id device int32 [n] (required), pos device int8 [n][npad][2] (npad 4 / 8 / 16 / 32; only the first N movables of a
 *   row are read into the key), mask device uint8 [n] or NULL.  Outputs and conventions are pw_search_table_query's: index
 *   (row within the item's table) -1 / cost -2 / acts 0 for a state that is not in the table (or has a coordinate outside
 *   0 .. 15 or the grid), cost -1 at a dead end.  Masked items and items whose puzzle has no STORED table in this handle
 *   (status other than 0, not in `puzzles`, id outside the set) are LEFT UNTOUCHED, so per-puzzle tables fill the same outputs.
 *   A puzzle listed twice is answered from its higher item.
 * Every argument check returns PW_EINVAL before any launch and names the function (null handle, n < 1, null puzzle_id / pos,
 * npad, rows_cap < 0, no run yet).
 * Memory: 27 bytes per row of pool (8 key + 16 succ + 2 cost + 1 acts) and 4 bytes per lookup slot -- a power of two
 * >= 2 x states (at least 16) slots per stored item, reserved as 4 slots per row + 16 per item: at most 43 bytes per row
 * of rows_cap; 37 bytes per item; 4 bytes per puzzle of the set.  The engine's slabs (shared with pw_search_batch): per
 * persistent workgroup 26 bytes per state of max_states_each + 12 bytes per slot of the 2^16 / 2^20 / ... closed-set levels. */
typedef struct PwSolveBatch PwSolveBatch;
int pw_solve_batch_create(PwEngine* e, int64_t rows_cap, PwSolveBatch** out);
void pw_solve_batch_destroy(PwSolveBatch* b);
int pw_solve_batch_run(PwSolveBatch* b, const int32_t* puzzles, int32_t n, int64_t max_states_each, void* stream);
/* device pointers (any may be NULL); returns the number of items of the last run */
int pw_solve_batch_results(PwSolveBatch* b, const uint8_t** status, const int32_t** summary, const int64_t** row_off);
/* the same arrays copied into the caller's device buffers [n], [n][5], [n] (any may be NULL), asynchronous on `stream` */
int pw_solve_batch_copy_results(PwSolveBatch* b, uint8_t* status, int32_t* summary, int64_t* row_off, void* stream);
int pw_solve_batch_totals(PwSolveBatch* b, int64_t totals[3], void* stream);
int pw_solve_batch_read(PwSolveBatch* b, int32_t item, int64_t first, int64_t count, uint64_t* key, int32_t* succ,
                        uint16_t* cost, uint8_t* acts, void* stream);
int pw_solve_batch_query(PwSolveBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                         int32_t n, int32_t* index, int32_t* cost, uint8_t* acts, void* stream);

/* Drawing from the cost-to-go tables on the device (csrc/pw_table_sample.inc): curriculum start states and optimal plans.
 * Every entry point has a pw_solve_batch_* form (all stored tables of the handle's last run, a MIXED batch, puzzle_id
 * required) and a pw_search_table_* form (the one table of a solved search; puzzle_id may be NULL = every item is of the
 * table's puzzle).  Each returns a status; every argument check returns PW_EINVAL before any launch and names the function.
 *
 * ..._index: the COST INDEX of every stored table, built on demand, idempotent, discarded by the next pw_solve_batch_run /
 *   pw_search_begin / destroy.  Per table:
 *     rows_by_cost  int32 [rows]           a permutation of the table's rows: all rows of cost 0, then cost 1, ... max_cost,
 *                                          then the dead ends (0xFFFF) as the last bucket
 *     cost_start    uint32 [max_cost + 3]  bucket c is [cost_start[c], cost_start[c + 1]); the dead ends are bucket
 *                                          max_cost + 1; the last entry is the number of rows
 *   Histogram, scan, scatter with atomics -- three launches for all tables of the handle.  The order INSIDE a bucket is
 *   whatever the build leaves and may differ from build to build (like pw_solve_batch_run's row numbers); it is fixed once
 *   built.  The batch form synchronises `stream` once when the run's summaries are not on the host yet (they size the
 *   arrays); both forms allocate.  Memory: 4 bytes per row (the batch form: per row of rows_cap) plus 4 bytes per bucket
 *   (max_cost + 3 per stored table), and 8 bytes per item of the batch.
 * ..._index_read: one table's two arrays copied into caller device buffers (either may be NULL), asynchronous on `stream`.
 *
 * ..._sample: ONE launch, no allocation, no synchronisation (capturable); the index must exist.  One start state per
 *   environment, drawn uniformly from the states of its puzzle whose cost-to-go lies in a band:
 *     puzzle_id  device int32 [n]            mask  device uint8 [n] or NULL: 0 skips an environment
 *     counter    device uint32 [n]           draws so far, per environment
 *     band       lo_n == hi_n == NULL: the scalars lo, hi (0 <= lo <= hi); else device int32 [n] each, hi_n[i] < lo_n[i]
 *                read as hi_n[i] = lo_n[i]
 *     pos        device int8 [n][npad][2]    npad 4 / 8 / 16 / 32 (the search form: >= the puzzle's number of movables)
 *     steps      device int32 [n]            term, trunc  device uint8 [n] or NULL
 *     out_row, out_cost  device int32 [n]
 *   Masked environments and environments whose puzzle has no stored, indexed table in the handle are LEFT ENTIRELY UNTOUCHED,
 *   the counter included (pw_solve_batch_query's convention: several tables fill one batch).  Otherwise the band is clamped to
 *   [0, max_cost] (lo > max_cost: lo = hi = max_cost; dead ends are never drawn).  A table without a finite-cost row gives
 *   out_row = out_cost = -1 and leaves everything else untouched.  Else
 *     counter[i] += 1;  r = mix64(seed ^ PW_TABLE_K_SAMPLE, i, counter[i])   (pw_mix64, K_SAMPLE = 0xA0761D6478BD642F)
 *     count = cost_start[hi + 1] - cost_start[lo];  u = floor(r * count / 2^64);  row = rows_by_cost[cost_start[lo] + u]
 *   and the environment is written as pw_reset writes it: the row's state in pos (zeros from the puzzle's N to npad - 1),
 *   steps = 0, term = trunc = 0; out_row = row, out_cost = its cost.
 *
 * ..._plans: ONE launch (capturable): a shortest plan from every given row (the batch form needs no index).
 *     index      device int32 [n] rows, as the query returns them         tie  0 / 1         plan_cap >= 1
 *     plans      device uint8 [n][plan_cap]                                plan_len  device int32 [n]
 *   One thread per item walks acts / succ down to cost 0.  tie 0 takes the lowest optimal action at every step; tie 1 takes,
 *   at step t, the j-th set bit of acts & 15 with k = popcount(acts & 15) and
 *     j = floor(mix64(seed ^ PW_TABLE_K_PLAN, i, t) * k / 2^64)              (K_PLAN = 0xE7037ED1A0B428DB)
 *   plan_len is the row's cost when 0 <= cost <= plan_cap; -1 for index < 0 (or beyond the table), a dead end, or a puzzle
 *   without a stored table here (plans untouched); -2 when the cost exceeds plan_cap (nothing is written).  Masked items are
 *   untouched. */
int pw_solve_batch_index(PwSolveBatch* b, void* stream);
int pw_solve_batch_index_read(PwSolveBatch* b, int32_t item, int32_t* rows_by_cost, uint32_t* cost_start, void* stream);
int pw_solve_batch_sample(PwSolveBatch* b, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad, uint64_t seed,
                          uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n, int8_t* pos,
                          int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_row, int32_t* out_cost, void* stream);
int pw_solve_batch_plans(PwSolveBatch* b, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                         int32_t tie, uint64_t seed, uint8_t* plans, int32_t plan_cap, int32_t* plan_len, void* stream);
int pw_search_table_index(PwSearch* s, void* stream);
int pw_search_table_index_read(PwSearch* s, int32_t* rows_by_cost, uint32_t* cost_start, void* stream);
int pw_search_table_sample(PwSearch* s, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad, uint64_t seed,
                           uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n, int8_t* pos,
                           int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_row, int32_t* out_cost, void* stream);
int pw_search_table_plans(PwSearch* s, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                          int32_t tie, uint64_t seed, uint8_t* plans, int32_t plan_cap, int32_t* plan_len, void* stream);

/* ---------------------------------------------------------- recursive graph distance (RGD) heuristic
 * RecursiveGraphDistanceHeuristic::estimate_cost_to_goal (cpp/src/heuristics/recursive_graph_distance.cc:43-252) for a
 * whole array of states of ONE puzzle of an engine's set.
 *
 * pw_puzzle_movement_graph: the feasible-movement graph of movable `obj` (domain_transition_graph.cc:113-216), host only.
 *   masks  host uint8 [height][width]: bit a (0..3 = L, R, U, D) = an edge from (x, y) in action a's direction,
 *          bit 4 = (x, y) is a node (every start position is one, edgeless or not).
 *
 * pw_rgd_create builds the graphs of every movable, uploads them and computes on the device the shortest-path length
 * between every pair of nodes of every graph (PathDistances::getDistance, domain_transition_graph.cc:218-300): one
 * wavefront per (movable, target) runs a breadth-first search over the reversed graph, one grid row per lane.  One device
 * allocation of sum over movables of nodes^2 * 2 bytes plus small tables; PW_ELIMIT above PW_RGD_MAX_BYTES.  Synchronous.
 *   fewest_tools  1: the reference default (recursive_graph_distance.h:179, what run_planner uses); 0: every goal's cost is
 *                 searched at pushing depth N - 2 (recursive_graph_distance.cc:53-58)
 *   budget        recursion frames (calls of get_recursive_pushing_cost) one state may take; 0 = PW_RGD_DEFAULT_BUDGET.
 *                 A state that needs more gets NaN and counts in pw_rgd_exceeded.  Each frame costs a few dozen dependent
 *                 table reads of one lane, so the budget is what bounds a launch: at 65 536 frames one launch of 2^20
 *                 full-depth states of a Level-1 puzzle with 11 movables ran 144 s (profiles/rgd_eval.txt); fewest-tools
 *                 states on Level 1 stay below 4 096.
 *
 * pw_rgd_eval: cost[k] = estimate_cost_to_goal of states[k] (+inf: provably no way to the goal), bit-identical to the
 *   reference.  states device int32 [count][N] Position2D (x * 10000 + y), pw_expand4's format; cost device float [count].
 *   One deviation: a state with a movable off its own graph gets NaN, where the reference throws from .at() (states
 *   reachable from the initial state never are).  Asynchronous on `stream`: no allocation, no synchronisation (capturable).
 * pw_rgd_distances: d[k] = the graph distance of movable `obj` from src[k] to dst[k] (device int32 Position2D in, device
 *   float out): 0 when src == dst is a node, +inf when dst is not a node or cannot be reached.  Asynchronous.
 * pw_rgd_exceeded: states that ran out of budget since pw_rgd_create (synchronises `stream`). */
#define PW_RGD_MAX_BYTES (1ll << 30)
#define PW_RGD_DEFAULT_BUDGET (1ll << 12)
typedef struct PwRgd PwRgd;
int pw_puzzle_movement_graph(const PwPuzzle* p, int32_t obj, uint8_t* masks);
int pw_rgd_create(PwEngine* e, int32_t puzzle, int32_t fewest_tools, int64_t budget, PwRgd** out);
void pw_rgd_destroy(PwRgd* r);
int pw_rgd_eval(PwRgd* r, const int32_t* states, float* cost, int32_t count, void* stream);
int pw_rgd_distances(PwRgd* r, int32_t obj, const int32_t* src, const int32_t* dst, float* d, int32_t count,
                     void* stream);
int64_t pw_rgd_exceeded(PwRgd* r, void* stream);

/* Best-first planner: the reference's run_planner (best_first_search.h:45-98 with a BucketPriorityQueue, run_planner.cc:37-61)
 * generalised to pop `batch` = K states per round.  At K = 1 it is the reference algorithm.
 *   mode     PW_PLAN_RGD: key = RGD cost (fewest tools); PW_PLAN_N_RGD: key = float(novelty * 1e6f) + cost (WeightedSumHeuristic).
 *            Lowest key first, LIFO within a key (the newest state, the highest store index, pops first); +inf after every finite
 *            key, NaN (an RGD budget overrun, counted in info[6]) last.  A finite cost at or above the bucket range (RGD: 2^22;
 *            N+RGD: 10^6, where the key stops being a bijection of (novelty, cost)) ends pw_planner_run with PW_ELIMIT.
 *   round    pop up to K states; expand each with the 4 actions of its action group; candidates in (pop rank, position in the
 *            group) order; a candidate is new when its state is not stored and no earlier candidate holds it; new states are
 *            stored in that order; the first new goal ends the search (solved), else every new state is scored (novelty
 *            tables in that order, then RGD) and pushed in that order.  A round is not started when store size + 4 K >
 *            max_states (status limit), nor when the queue is empty (exhausted).
 *   flags    PW_PLAN_ACTIONS_REFERENCE: RandomActionIterator (1000 std::shuffle permutations, std::default_random_engine(42));
 *            the state popped p-th (from 0) takes group (p + 1) mod 1000.  PW_PLAN_ACTIONS_FIXED: L, R, U, D for every parent.
 *   memory   a PwSearch of max_states with 4 K candidates per pass (pw_search_create's formula: the store, about max_states *
 *            (2N + 5) bytes, the closed set, 8 bytes per slot of a power of two >= 2 (max_states + 4 K), and K * (8 N + 52)
 *            bytes of candidates), a PwRgd (<= 1 GiB), 16 bytes per state of queue entries and segments (+ 1 in N+RGD mode),
 *            4 bytes per bucket (2^22 + 2, or 3 * 10^6 + 2 in N+RGD mode) + 1 bit per bucket of occupancy, K * (16 N + 97)
 *            bytes of round scratch (+ 20 in N+RGD mode) + the rocPRIM radix sort's temporary storage for 4 K pairs and, in
 *            N+RGD mode, a PwNovelty (4 N D + 2 N (N - 1) D^2 bytes, D = width * height).
 * pw_planner_begin: from `start` (host Position2D [N]) or the initial state; a start state that is a goal is solved at once
 *   (empty plan).  pw_planner_run: at most max_rounds rounds (<= 0: until the status is not running), enqueued without
 *   synchronising; the status is read once per group of rounds (pw_planner_set_sync_rounds, 0 = 16), which changes nothing
 *   in the result (after the search ends, the rest of a group costs one radix sort of 4 K keys per round, the other
 *   kernels return at once).  info: [0] status, [1] rounds, [2] expanded (states popped), [3] visited (the start state and every new
 *   state numbered before the goal), [4] open (states in the queue), [5] goal store index or -1, [6] RGD budget overruns,
 *   [7] store size.  pw_planner_plan: the plan to the goal, like pw_search_plan.  pw_planner_max_key: the largest finite
 *   key pushed so far.  pw_planner_action_groups: the 1000 reference action groups (host only; returns 1000). */
#define PW_PLAN_RGD 0
#define PW_PLAN_N_RGD 1
#define PW_PLAN_ACTIONS_REFERENCE 0
#define PW_PLAN_ACTIONS_FIXED 1
#define PW_PLAN_RUNNING 0
#define PW_PLAN_SOLVED 1
#define PW_PLAN_EXHAUSTED 2
#define PW_PLAN_LIMIT 3
typedef struct PwPlanner PwPlanner;
int pw_planner_create(PwEngine* e, int32_t puzzle, int32_t mode, int64_t max_states, int32_t batch, int32_t flags,
                      int64_t rgd_budget, PwPlanner** out);
void pw_planner_destroy(PwPlanner* p);
int pw_planner_set_sync_rounds(PwPlanner* p, int32_t rounds);
int pw_planner_begin(PwPlanner* p, const int32_t* start, void* stream);
int pw_planner_run(PwPlanner* p, int64_t max_rounds, int64_t info[8], void* stream);
int pw_planner_plan(PwPlanner* p, uint8_t* actions, int32_t cap, void* stream);
int pw_planner_max_key(PwPlanner* p, float* out, void* stream);
int pw_planner_action_groups(uint8_t* out);

/* Batched best-first search (K9): the planner runs of MANY puzzles in ONE launch.  Persistent workgroups of one wavefront take
 * the items off a device counter and run each one's whole search inside the kernel.  Item i's info[0..7] and plan equal
 * pw_planner_create(e, puzzles[i], mode, max_states, batch, flags, rgd_budget) + begin(initial state) + run(max_rounds),
 * as long as no finite cost reaches cost_range.
 *   puzzles     host int32 [n] set indices of the items, or NULL (0 .. n - 1); an index may repeat
 *   batch       K, 1 .. 64
 *   max_states  1 .. 2^28 states per item (every workgroup owns a slab of that many)
 *   cost_range  0 (65536) or 1 .. 65536: finite RGD costs 0 .. cost_range - 1 have a bucket; a larger one ends the item with
 *               PW_PLAN_RANGE (pw_planner's ranges are 2^22 and 10^6)
 *   memory      per workgroup: max_states * (4 ceil(N / 2) + 9) bytes + 8 bytes per slot of the closed set (a power of two
 *               >= 2 max_states) + 4 bytes per bucket + in N+RGD mode 1 bit per novelty atom (N D + N (N - 1) / 2 D^2,
 *               D = width * height; N, D of the largest item); one workgroup per item, at most 2 per CU, fewer when their
 *               slabs would take more than a quarter of the free device memory.  Plus one PwRgd per item.
 * pw_plan_batch_run: one asynchronous launch on `stream`.  info: device int64 [n][PW_PLAN_BATCH_INFO] (pw_planner_run's
 *   eight values, then [8] the item's search time on the device in nanoseconds); plans: device uint8 [n][plan_cap] or NULL,
 *   plan_len: device int32 [n] (length of the plan, -1 without one; a plan longer than plan_cap is cut), or NULL.
 *   max_rounds <= 0: no round limit.  time_limit: seconds per item (0 = none), read on the device's constant clock before
 *   every round; an item past it ends with PW_PLAN_TIMEOUT.
 * pw_plan_batch_cancel: every launch of this handle made so far stops soon: running items after at most 32 more rounds, with
 *   status PW_PLAN_RUNNING and the counts they reached; items not started yet report PW_PLAN_RUNNING with 0 rounds.  The
 *   cancel word lives in pinned host memory: no stream is involved. */
#define PW_PLAN_TIMEOUT 4
#define PW_PLAN_RANGE 5
#define PW_PLAN_SKIPPED 6
#define PW_PLAN_BATCH_INFO 9
typedef struct PwPlanBatch PwPlanBatch;
int pw_plan_batch_create(PwEngine* e, const int32_t* puzzles, int32_t n, int32_t mode, int64_t max_states, int32_t batch,
                         int32_t flags, int64_t rgd_budget, int32_t cost_range, PwPlanBatch** out);
int pw_plan_batch_run(PwPlanBatch* b, int64_t max_rounds, double time_limit, int64_t* info, uint8_t* plans, int32_t* plan_len,
                      int32_t plan_cap, void* stream);
/* pw_plan_batch_run_states: the same searches from given states -- e.g. the live states of a batch of environments.  Item i
 * of the run is puzzle_id[i] from start state pos[i].  Item i's info[0..7] and plan equal pw_planner_create(e, puzzle_id[i],
 * mode, max_states, batch, flags, rgd_budget) + pw_planner_begin(start = pos[i]) + pw_planner_run(max_rounds) with the
 * handle's settings, as long as no finite cost reaches cost_range: the reference's best_first_search on the puzzle with its
 * initial state replaced by pos[i].  All arrays live in device memory; nothing is read on the host, so the call is one
 * asynchronous launch on `stream` that may follow a pw_step on the same stream without a synchronisation.
 *   puzzle_id     int32 [n] set indices of the handle's engine (a VecPushWorld's puzzle_id as it is)
 *   pos           int8 [n][npad][2], x then y per movable: the engine's state layout (pw_engine_npad); padding is not read
 *   mask          uint8 [n] or NULL: 0 skips the item
 *   first_action  int8 [n] or NULL: the plan's first action when the item is solved with a non-empty plan, -1 otherwise
 *                 (a start at its goal is solved with an empty plan: -1)
 *   info, plans, plan_len, plan_cap, max_rounds, time_limit: as for pw_plan_batch_run, with n rows
 * An item is PW_PLAN_SKIPPED (info[0] = 6, info[1..8] = 0, plan_len -1, first_action -1) when it is masked out, its puzzle
 * id is outside the set, the handle did not prepare that puzzle (pw_plan_batch_create's `puzzles`; the first item naming a
 * puzzle lends it its tables) or a movable lies outside its grid (pw_validate_state's range test).  Walls and overlaps are
 * not checked, as the reference does not check them.  Closed-set tags: a run uses n of them.
 * The handle has at most one workgroup per prepared item; the first run with more items adds workgroups up to two per CU
 * (within a quarter of the free memory), which waits for the device once.
 * PW_EINVAL before any launch: n < 1, npad not 4 / 8 / 16 / 32, a null puzzle_id / pos / info, plans without plan_len,
 * a null handle, npad below the largest prepared puzzle's number of movables. */
int pw_plan_batch_run_states(PwPlanBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                             int32_t n, int64_t max_rounds, double time_limit, int64_t* info, uint8_t* plans,
                             int32_t* plan_len, int32_t plan_cap, int8_t* first_action, void* stream);
int pw_plan_batch_cancel(PwPlanBatch* b);
void pw_plan_batch_destroy(PwPlanBatch* b);

/* Plan replay (K11): ONE ragged replay of a whole batch of plans on the device -- the reference's is_valid_plan verdict
 * (puzzle.py:413-424) per plan, and every step of every accepted plan as a row of flat device arrays (state, action, reward,
 * done), ready for pw_render / pw_render_cells over (row_puzzle_id, row_pos).  The inputs are device memory in the formats
 * pw_plan_batch_run / pw_plan_batch_run_states write, so a planner's outputs go in as they are, on the same stream.
 *   puzzle_id   int32 [n] set indices of the engine
 *   pos         int8 [n][npad][2] start states in the engine's layout, or NULL: every item starts from its puzzle's initial state
 *   npad        4, 8, 16 or 32, at least the set's largest number of movables (pw_engine_npad fits)
 *   plans       uint8 [n][plan_cap]; plan_len int32 [n]; plan_cap 1 .. PW_PLAN_MAX_ACTIONS
 *   mask        uint8 [n] or NULL: 0 skips the item
 * pw_plan_replay_check replays every item and writes
 *   verdict     int8 [n]:
 *     PW_REPLAY_VALID     the goal holds after the last action and in no earlier state: is_valid_plan from the given start.  As
 *                         there, the empty plan is valid exactly when the start is a goal, and any longer plan from a start
 *                         that is a goal is PW_REPLAY_EARLY.
 *     PW_REPLAY_NOT_GOAL  neither the final state nor an earlier one is a goal
 *     PW_REPLAY_EARLY     some state before the last is a goal
 *     PW_REPLAY_NONE      plan_len < 0
 *     PW_REPLAY_CUT       plan_len > plan_cap: the stored plan is incomplete, nothing is replayed
 *     PW_REPLAY_SKIPPED   the item is masked out, its id is outside the set or a movable lies outside its grid
 *                         (pw_plan_batch_run_states' range test; nothing further of the item is read), or a plan byte is not in 0..3
 *   first_goal  int32 [n] or NULL: index of the first goal state (0 = the start), -1 when there is none or nothing was replayed
 *   final_pos   int8 [n][npad][2] or NULL: the state after the last action (zeros for an item that was not replayed)
 *   offset      int64 [n + 1]: exclusive prefix sum of the rows every item will emit -- plan_len when the item is included,
 *               else 0; offset[n] = the total.  include = PW_REPLAY_INCLUDE_VALID keeps the VALID items,
 *               PW_REPLAY_INCLUDE_REPLAYED the VALID, NOT_GOAL and EARLY ones.
 * pw_plan_replay_emit takes the same inputs with the `verdict` and `offset` of the check and writes row offset[i] + t of every
 * included item i, t < plan_len[i] (any output may be NULL):
 *   row_item / row_t / row_puzzle_id int32 [cap]; row_pos int8 [cap][npad][2]: the state BEFORE the action, padding zeroed as
 *   pw_render expects; row_action uint8 [cap]; row_reward float64 [cap] and row_done uint8 [cap]: exactly pw_step's reward and
 *   `terminated` of that step (10.0 when the next state is a goal, else the change of goals achieved - 0.01);
 *   row_next_pos int8 [cap][npad][2]: the state after it.
 *   Rows at or beyond `cap` are not written; *dropped (device int64, or NULL) receives how many were left out.
 * Both are asynchronous on `stream` (a replay is one launch; the check adds rocPRIM's scan) and read nothing on the host.  The
 * engine keeps a small workspace that grows with n (the first call of a size allocates).
 * PW_EINVAL before any launch, pw_last_error naming the argument: n < 1; npad not 4 / 8 / 16 / 32; a null puzzle_id, plans,
 * plan_len, verdict or offset; plan_cap outside 1 .. PW_PLAN_MAX_ACTIONS; an unknown include; cap < 0; a null engine; npad below
 * the set's largest number of movables. */
#define PW_REPLAY_VALID 1
#define PW_REPLAY_NOT_GOAL 0
#define PW_REPLAY_EARLY 2
#define PW_REPLAY_NONE (-1)
#define PW_REPLAY_CUT (-2)
#define PW_REPLAY_SKIPPED (-3)
#define PW_REPLAY_INCLUDE_VALID 0
#define PW_REPLAY_INCLUDE_REPLAYED 1
int pw_plan_replay_check(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* plans,
                         const int32_t* plan_len, int32_t plan_cap, const uint8_t* mask, int32_t n, int32_t include,
                         int8_t* verdict, int32_t* first_goal, int8_t* final_pos, int64_t* offset, void* stream);
int pw_plan_replay_emit(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* plans,
                        const int32_t* plan_len, int32_t plan_cap, const uint8_t* mask, int32_t n, int32_t include,
                        const int8_t* verdict, const int64_t* offset, int64_t cap, int32_t* row_item, int32_t* row_t,
                        int32_t* row_puzzle_id, int8_t* row_pos, uint8_t* row_action, double* row_reward, uint8_t* row_done,
                        int8_t* row_next_pos, int64_t* dropped, void* stream);

/* Walk regions and push moves (K15): what a search over pushes, a push-level action space or an "is any push available" mask
 * needs, for a whole batch of states in one launch.  Everything is defined through the step function, for states with
 * overlaps too.  Take a state s with agent position q0 (the origin of the agent's bounding box):
 *   walk move (q, a)   stepping s with the agent placed at q by action a moves the agent and nothing else
 *   walk region R(s)   the agent positions reachable from q0 by walk moves, the other movables fixed; dist(q) is the
 *                      breadth-first distance, dist(q0) = 0.  A position at which the agent leaves its grid is not in R.
 *   parent(q), q != q0 the lowest action a for which q' = q - d_a is in R, dist(q') = dist(q) - 1 and (q', a) is a walk move
 *   push move (q, a)   q in R and that step moves the agent and at least one other movable; its successor is the state after
 *                      the step.  A step that moves nothing is neither.
 *   canon(s)           the position of R(s) smallest in (y, x) order
 * puzzle_id / pos / npad / mask as pw_plan_replay_check (pos NULL: the initial states; nothing beyond a puzzle's N movables
 * is read).  pw_walk_regions writes
 *   region_size int32 [n]      positions of R (>= 1); -1 for an item that is masked out, has an id outside the set or a movable
 *                              outside its grid (nothing further of it is read)
 *   canon       int8 [n][2] or NULL: canon(s) as (x, y), zeros for a skipped item
 *   offset      int64 [n + 1]  exclusive prefix sum of the push moves per item (0 for a skipped one); offset[n] = the total
 *   walk_map    uint16 [n][map_h][map_w] or NULL; map_h / map_w at least the set's largest dimensions (pw_puzzleset_max_dims)
 *               and at most PW_MAX_DIM.  Entry [y][x]: 0xFFFF where (x, y) is not in R, else dist | parent << 12 (q0 holds 0;
 *               a board has at most 62 x 62 cells inside its border, so dist fits 12 bits).  Every entry of every item's map
 *               is written: 2 * map_h * map_w bytes per item.
 * pw_walk_pushes takes the same inputs and the offset of the first call, recomputes, and writes row offset[i] + k for the k-th
 * push move of item i, ordered by (y, x) of the agent position it starts from, then by action (any output may be NULL):
 *   row_item int32 [cap]; row_from int8 [cap][2] the position q; row_action uint8 [cap]; row_walk int32 [cap] dist(q);
 *   row_moved uint32 [cap] bit j = movable j moved (as pw_expand4); row_goal uint8 [cap] 1 when the successor is a goal state;
 *   row_next_pos int8 [cap][npad][2] the successor, padding zeroed as pw_render and pw_validate_state require.
 *   Rows at or beyond `cap` are not written; *dropped (device int64, or NULL) receives how many were left out.
 * Both are asynchronous on `stream` (one launch each; the first adds a fill of the maps and rocPRIM's scan) and read nothing on
 * the host; they share the plan replay's workspace.  pos, canon, row_from and row_next_pos are read and written as 2-byte (x, y)
 * pairs: they must be 2-byte aligned (as pos and the rows of pw_plan_replay_emit; any device allocation is).
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: n < 1; npad not 4 / 8 / 16 / 32; a null
 * puzzle_id, offset, region_size or engine; cap < 0; map_h / map_w outside 1 .. PW_MAX_DIM or below the set's largest
 * dimensions when walk_map is given; npad below the set's largest number of movables. */
int pw_walk_regions(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask, int32_t n,
                    int32_t* region_size, int8_t* canon, int64_t* offset, uint16_t* walk_map, int32_t map_h, int32_t map_w,
                    void* stream);
int pw_walk_pushes(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask, int32_t n,
                   const int64_t* offset, int64_t cap, int32_t* row_item, int8_t* row_from, uint8_t* row_action,
                   int32_t* row_walk, uint32_t* row_moved, uint8_t* row_goal, int8_t* row_next_pos, int64_t* dropped,
                   void* stream);

/* Stepping by pushes (K19): the push-level action space of K15 acted in.  A choice (from, a) per environment -- an agent
 * position (x, y) and a uint8 action -- is VALID when a is in 0..3, from lies in the walk region R of the environment's state
 * and (from, a) is a push move of it.  The macro step of a valid choice is pw_step applied with the actions
 * L = path(R, from) + [a] in turn (the parent actions of pw_walk_regions from the agent's position to `from`, then the push:
 * dist(from) + 1 actions), without autoreset inside; it ends after the first step that returns terminated | truncated, or
 * after the last action.  pw_step_push performs it for a whole batch in one launch and writes
 *   pos, steps, terminated, truncated   what the last executed pw_step left
 *   reward  double [batch] or NULL      the sum of the executed steps' rewards, added in execution order ((r1 + r2) + r3) + ...
 *   dgoals  int8 [batch] or NULL        the sum of the executed steps' dgoals
 *   moves   int32 [batch] or NULL       the number of primitive steps executed
 *   status  int8 [batch] or NULL        PW_PUSH_DONE: the push itself was executed; PW_PUSH_CUT: the macro step ended during the
 *                                       walk -- max_steps was reached (the agent stands on the path where it had got to), or
 *                                       the state was a goal state already (the first walking step returns terminated)
 * A choice that is not valid is REFUSED: pos, steps, terminated and truncated stay as they were, reward 0.0, dgoals 0, moves 0,
 * status PW_PUSH_REFUSED.  That covers a position outside the grid or outside R, a walk move, a move that displaces nothing, an
 * action outside 0..3 (PUSH_NONE = 0xFF, the best push of a goal state or a dead end, is harmless to feed back in), a puzzle id
 * outside the set and a movable outside its grid.  There are no 0xFF flags and no bad-action count in this action space.
 * With PW_STEP_AUTORESET an environment whose terminated | truncated is set on entry is reset exactly as pw_step resets it (the
 * initial state of puzzle_id[e], steps 0, flags 0, reward 0.0): moves 0, status PW_PUSH_RESET, the choice is not read.
 * The counters of pw_counters advance as the `moves` executed primitive steps would have advanced them (a reset or a refusal
 * executes none).  An environment without any push move can never be stepped by this call: that is the caller's business
 * (status, pw_push_mask, pw_reset with a mask).
 * pos is in the engine's layout (pw_engine_npad), as for pw_step.  Asynchronous on `stream`, one launch, nothing is read on the
 * host.  Workspace: none per environment -- the path ancestor a cut needs lives in LDS -- so the call allocates nothing at any
 * batch size once the engine's replay workspace exists (4 KB of item counters, shared with pw_plan_replay_* and pw_walk_*,
 * allocated by the first call of any of them; it only ever grows on their demand).
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: a null engine, puzzle_id, push_from,
 * push_action, pos, steps, terminated or truncated; batch < 1; an engine with an open mailbox.
 *
 * pw_push_mask writes the dense mask of that action space, inputs and checks as pw_walk_regions (pos NULL: the initial states;
 * map_h / map_w at least the set's largest dimensions; npad at least its movables): entry [y][x] of item i has bit a set exactly
 * when ((x, y), a) is a push move of item i, 0 everywhere else and for a skipped item; every entry of every item is written.
 * num_pushes[i] is the popcount of item i's entries (offset[i + 1] - offset[i] of pw_walk_regions).  One fill and one launch:
 * the region pass of pw_walk_regions with its push boards written out.  PW_EINVAL as pw_walk_regions, and for a null push_mask. */
#define PW_PUSH_REFUSED 0
#define PW_PUSH_DONE 1
#define PW_PUSH_CUT 2
#define PW_PUSH_RESET 3
int pw_step_push(PwEngine* e, const int32_t* puzzle_id, const int8_t* push_from /* [B][2] (x, y) */,
                 const uint8_t* push_action /* [B] */, int8_t* pos, int32_t* steps, double* reward, int8_t* dgoals,
                 uint8_t* terminated, uint8_t* truncated, int32_t* moves, int8_t* status,
                 int32_t batch, uint32_t flags, void* stream);
int pw_push_mask(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask, int32_t n,
                 uint8_t* push_mask /* [n][map_h][map_w] */, int32_t* num_pushes /* [n] or NULL */,
                 int32_t map_h, int32_t map_w, void* stream);

/* Stepping by pushes with the mask kept (K23): what a learner in pushes calls once per step.  pw_step_push_mask steps a batch as
 * pw_step_push does and leaves, per environment, the push mask and the walk map of the state that is left -- in one launch, and
 * with one flood per environment where pw_step_push followed by pw_push_mask floods twice.
 * The six buffers push_mask .. view_id are the VIEW of an environment.  The caller owns them; the library keeps no state:
 *   push_mask   uint8  [batch][map_h][map_w]   as pw_push_mask writes it
 *   num_pushes  int32  [batch]                 as pw_push_mask writes it
 *   walk_map    uint16 [batch][map_h][map_w]   as pw_walk_regions writes it
 *   region_size int32  [batch]                 as pw_walk_regions writes it
 *   view_pos    int8   [batch][npad][2]        the first N (x, y) pairs of the state the view describes, zeros beyond
 *   view_id     int32  [batch]                 the puzzle id of that state; -1: no state
 * The view of environment e is CURRENT when view_id[e] == puzzle_id[e], an index into the set, and the first N pairs of
 * view_pos[e] equal those of pos[e], N the puzzle's number of movables; nothing beyond N is compared.  Filling view_id with -1
 * invalidates every view; a buffer fresh from the allocator must be invalidated that way.
 * Per environment:
 *   1. Step phase.  pos, steps, reward, dgoals, terminated, truncated, moves and status are bit for bit what pw_step_push writes
 *      for the same inputs and flags (the reset under PW_STEP_AUTORESET, every refusal, the cuts, the sequential float64 reward
 *      sum), and pw_counters advances as it does there.  reward, dgoals, moves and status may be NULL.
 *   2. View phase.  The view of e then describes the state that was left: push_mask[e] / num_pushes[e] equal what pw_push_mask,
 *      walk_map[e] / region_size[e] what pw_walk_regions writes for it; every entry is written.  A skipped item (an id outside
 *      the set, a movable outside its grid) gets zeros in the mask, 0xFFFF in the map, num_pushes 0, region_size -1, view_id -1
 *      and zeros in view_pos.  Otherwise view_pos[e] holds the first N pairs of the new pos[e] and zeros beyond, view_id[e] the id.
 *   3. PW_PUSH_END_STUCK (flags, next to PW_STEP_AUTORESET; read by this function only) applies after the view phase to every
 *      environment with num_pushes[e] == 0 and neither terminated nor truncated set: truncated[e] = 1, and episodes_ended of
 *      pw_counters advances by one for it.  status, reward and moves stay as they are.  With PW_STEP_AUTORESET the next call
 *      resets it.  Without the flag nothing of the kind happens.
 * How the view is used.  A current view replaces the step phase's flood: the choice (from, a) is valid exactly when a is in
 * 0..3, walk_map[from] != 0xFFFF and bit a of push_mask[from] is set; dist(from) is the entry's low 12 bits; the agent's position
 * at a max_steps cut is found by following the parent actions back from `from`; the push itself is one evaluation of the step
 * function's push set.  A stale view is rebuilt first, by one flood of the state on entry, and the same path follows.  A choice
 * refused on a current view costs no flood: state and view stay as they are.  So a call whose push_action is all PUSH_NONE
 * (0xFF), without PW_STEP_AUTORESET, is the "observe" operation: it rebuilds the stale views and steps nothing.
 * A view that is current by id and positions but whose contents were not written by this function is the caller's error; it can
 * lead to a wrong verdict, never to a read out of bounds or an endless loop: every position on the way back along the parents is
 * range-checked, the way is at most dist <= 4 095 links long, and a link that is 0xFFFF or whose dist does not drop by one makes
 * the view stale (it is rebuilt and the step goes on).
 * Asynchronous on `stream`: one launch behind the four-byte clear of an item counter, no fill of the view, no allocation once
 * the engine's replay workspace exists (shared, as for pw_step_push), nothing read on the host -- the call can be captured into
 * a graph.  pos and view_pos are read and written as 2-byte pairs.
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: everything pw_step_push refuses; a null
 * push_mask, num_pushes, walk_map, region_size, view_pos or view_id; map_h / map_w outside 1 .. PW_MAX_DIM or below the set's
 * largest dimensions. */
#define PW_PUSH_END_STUCK 0x100u
int pw_step_push_mask(PwEngine* e, const int32_t* puzzle_id, const int8_t* push_from /* [B][2] */,
                      const uint8_t* push_action /* [B] */, int8_t* pos, int32_t* steps, double* reward, int8_t* dgoals,
                      uint8_t* terminated, uint8_t* truncated, int32_t* moves, int8_t* status,
                      uint8_t* push_mask /* [B][map_h][map_w] */, int32_t* num_pushes /* [B] */,
                      uint16_t* walk_map /* [B][map_h][map_w] */, int32_t* region_size /* [B] */,
                      int8_t* view_pos /* [B][npad][2] */, int32_t* view_id /* [B] */,
                      int32_t map_h, int32_t map_w, int32_t batch, uint32_t flags, void* stream);

/* Pushes unrolled into primitive actions (K21): the bridge from the push level back to the move level.  Item i is a state s
 * (puzzle_id[i], pos[i]; pos NULL: the initial states, as pw_walk_regions) and a choice (from, a) = (push_from[i],
 * push_action[i]).  The choice is VALID by pw_step_push's rule, unchanged: a in 0..3, from in the walk region R(s), (from, a) a
 * push move.  Its unrolled sequence is
 *   L = path(R, from) + [a]
 * where path(R, from) is the parent actions of pw_walk_regions' map from the agent's position to `from`: the L of the
 * pw_step_push comment, so len(L) = dist(from) + 1 is in 1 .. 4096.  An item is REFUSED -- length -1, no byte written -- when
 * it is masked out (mask[i] == 0), its id is outside the set, a movable lies outside its grid, or its choice is not valid
 * (PUSH_NONE = 0xFF counts as not valid).
 * pw_push_unroll_count writes
 *   length  int32 [n]      len(L), or -1 for a refused item
 *   offset  int64 [n + 1]  the exclusive prefix sum of max(length, 0); offset[n] = the total number of actions
 * pw_push_unroll_write takes the same inputs and the offset of the first call, recomputes, and writes
 *   actions uint8 [cap]    actions[offset[i] + k] = L[k].  Bytes at or beyond `cap` are not written; *dropped (device int64, or
 *                          NULL) receives how many were left out.  actions may be NULL when cap is 0.
 * pw_push_unroll_plans gathers unrolled rows into plan arrays in exactly the format pw_plan_replay_check takes.  The rows
 * item_offset[j] .. item_offset[j + 1] - 1 (item_offset int64 [m + 1], ascending, within 0 .. rows) are the consecutive pushes
 * of plan j -- the layout of pw_push_search_table_emit -- and length int32 [rows], offset int64 [rows + 1], actions uint8 [cap]
 * are what count and write left for those rows:
 *   plan_len int32 [m]           the sum of the rows' lengths (offset[last + 1] - offset[first]: the spans of consecutive rows are
 *                                contiguous in `actions`); 0 for a plan without rows; -1 (PW_REPLAY_NONE) for a plan with a
 *                                refused row, with rows outside 0 .. rows, or with bytes at or beyond cap
 *   plans    uint8 [m][plan_cap] the first min(plan_len, plan_cap) actions of the plan; a plan longer than plan_cap keeps its
 *                                true plan_len (PW_REPLAY_CUT downstream).  Bytes beyond that are left as they were.
 * All three are asynchronous on `stream` and read nothing on the host; count and write are one launch each (count adds
 * rocPRIM's scan), the gather is one launch.  They use the engine's shared replay workspace only (the item counters, and the
 * scan's temporary storage, which the first call of a size allocates).  pos and push_from are read as 2-byte (x, y) pairs.
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: a null engine, puzzle_id, push_from,
 * push_action, length, offset, item_offset, plans or plan_len; null actions with cap > 0; n or m < 1; npad not 4 / 8 / 16 / 32 or
 * below the set's largest number of movables; cap or rows < 0; plan_cap outside 1 .. PW_PLAN_MAX_ACTIONS.
 * No kernel waits on another workgroup; there is no device assert; every loop is bounded by the items, the cells of a board
 * times four actions, or 4 095 layers. */
int pw_push_unroll_count(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad,
                         const int8_t* push_from /* [n][2] (x, y) */, const uint8_t* push_action /* [n] */,
                         const uint8_t* mask, int32_t n, int32_t* length, int64_t* offset, void* stream);
int pw_push_unroll_write(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const int8_t* push_from,
                         const uint8_t* push_action, const uint8_t* mask, int32_t n, const int64_t* offset, int64_t cap,
                         uint8_t* actions, int64_t* dropped, void* stream);
int pw_push_unroll_plans(PwEngine* e, const int64_t* item_offset, const int32_t* length, const int64_t* offset,
                         const uint8_t* actions, int64_t rows, int64_t cap, int32_t m, int32_t plan_cap, uint8_t* plans,
                         int32_t* plan_len, void* stream);

/* Breadth-first search over pushes with its closed set on the device (K16).  A node is a canonical state: the packed positions
 * with the agent's pair replaced by canon(s).  The store keeps, per node, the state as reached (the agent where the push left
 * it) and its canon; state 0 is the start.  Layer d + 1 holds the successors of the push moves of layer d's states: the states
 * in store order, a state's push moves in pw_walk_pushes' (y, x, action) order; a successor is appended when it lies inside
 * its grid, its canonical state is not in the closed set, and it is the first row in that order with that canonical state.
 * The numbering is therefore that of a sequential search and independent of PW_OPT_SEARCH_CHUNK (parents per pass, read at
 * creation; 0 = 2^16) and of the order in which workgroups ran.  The closed set is a table in HBM of fingerprint | store index
 * entries, a power of two of at least 2 (max_states + 1) slots; a fingerprint match is always confirmed against the canonical
 * state in the store, so two different canonical states are never merged and equal ones never both kept, at every number of
 * movables.  PW_OPT_PUSH_SEARCH_FP_BITS (read at creation) keeps fewer fingerprint bits and changes no result.
 * Links of a state: parent (store index, -1 for the start), from (the agent position the push started from), action (0xFF for
 * the start), walk (dist(from) in the parent's walk region), goal (1: a goal state).
 * With stop_at_goal the search ends in the first layer that holds a push move into a goal state: the successor of the first
 * such row is the last state of the store (states == goal index + 1) and the rows after it are not published; a start that is
 * a goal state ends it at once (pw_push_search_expand then returns PW_EINVAL).  Without, it runs on through goal states until
 * a layer is empty.  From a state with overlaps a push move can carry a movable out of its grid.  Such a successor is no
 * candidate of the closed set and is never appended -- unless it is that first goal row's: then it is still the last state of
 * the store, as reached, with canon (0, 0) and region size -1 (what pw_walk_regions gives a skipped item), and it is the one
 * state of a store that owns no entry of the closed set.
 * Device memory: 2 NP + 22 bytes per state of max_states (NP = the engine's padded number of movables) and 16 .. 32 bytes of
 * table; per push row of the largest pass 2 NP + 4 ceil(N / 2) + 52 bytes of workspace, which starts at 4 096 rows and grows on demand;
 * pw_push_search_begin clears the table (8 bytes per slot).  The search
 * owns its workspace: a pw_walk_regions call of the user's does not disturb it.  A state's walk region is flooded once, as a
 * successor: its region size and push count are kept in the store (8 of those bytes).
 * pw_push_search_expand waits once per pass for the pass's row count and once at the end of the layer.
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: a null handle, engine, out or info;
 * max_states outside 1 .. 2^31 - 1; a puzzle index outside the set; a start with a movable outside its grid; a range or an
 * index outside the store; a call before pw_push_search_begin.  PW_ELIMIT from pw_push_search_expand when the store is full:
 * the layer is incomplete, info is filled in, and every later call of it fails until the next pw_push_search_begin. */
#define PW_OPT_PUSH_SEARCH_FP_BITS 52 /* pw_push_search_create (read at creation): fingerprint bits of the closed set's entries, 1 .. 32
                                         (0 = default, 32).  With 1 or 2 almost every probe meets an equal fingerprint and the exact
                                         comparison decides: for tests */
typedef struct PwPushSearch PwPushSearch;
int  pw_push_search_create(PwEngine* e, int32_t puzzle, int64_t max_states, PwPushSearch** out);
void pw_push_search_destroy(PwPushSearch* s);
/* start: host int8 [N][2] (x, y) or NULL = the initial state.  PW_EINVAL for a movable outside its grid. */
int  pw_push_search_begin(PwPushSearch* s, const int8_t* start, int32_t stop_at_goal, void* stream);
/* one layer of pushes; synchronises.
   info[0] depth of the new layer
   info[1] states in it (0: exhausted)
   info[2] states in the store
   info[3] goal index, or -1
   info[4] push rows listed in this layer
   info[5] largest walk region seen so far */
int  pw_push_search_expand(PwPushSearch* s, int64_t info[6], void* stream);
/* device outputs, any may be NULL:
   pos int8 [count][npad][2], the state as reached, padding zeroed
   canon int8 [count][2] */
int  pw_push_search_read_states(PwPushSearch* s, int64_t first, int64_t count, int8_t* pos, int8_t* canon, void* stream);
int  pw_push_search_read_links(PwPushSearch* s, int64_t first, int64_t count, int32_t* parent, int8_t* from,
                               uint8_t* action, int32_t* walk, uint8_t* goal, void* stream);
/* Primitive actions from the start to state `index`, ending with the push that reached it.  The walks between pushes are the
   parent actions of pw_walk_regions' map.  Host buffer.  Returns the length (nothing written if > cap), or an error.
   pushes (may be NULL) receives the number of pushes on the chain. */
int  pw_push_search_plan(PwPushSearch* s, int64_t index, uint8_t* actions, int32_t cap, int32_t* pushes, void* stream);

/* Exact cost-to-go table over pushes (K18), on a PwPushSearch that has been EXHAUSTED: begun with stop_at_goal = 0, its last
 * pw_push_search_expand reported 0 new states, and the store did not overflow.  Let S be the number of states in the store.
 * Rows.  State i has npush[i] push rows, in pw_walk_pushes' (y, x, action) order, taken from the state as stored.  row_off
 * (int64 [S + 1]) is the exclusive scan of npush, R = row_off[S].  For row r of state i:
 *   succ[r]   int32     the store index of the canonical state of the row's successor; -1 when the successor lies outside its
 *                       grid (such rows exist from overlapping starts; K16 never appends them)
 *   from[r]   int8 [2], action[r] uint8: as pw_walk_pushes writes them
 *   flags[r]  uint8     bit 0 goal (row_goal), bit 1 optimal, bit 2 safe, as defined below
 *   A successor inside its grid that is missing from the closed set is an internal error: PW_EDEVICE, as in pw_search_solve.
 * Cost.  Cost is counted in PUSHES and is not a count of moves.  The value of a row is c(r) = 0 when its goal bit is set,
 * whatever succ[r] is; otherwise c(r) = cost[succ[r]] when succ[r] >= 0; otherwise c(r) is infinite.  cost[i] (int32) is 0 where
 * the store's goal[i] is 1; elsewhere it is 1 + min_r c(r) over the state's rows; it is -1 where that minimum is infinite: a
 * dead end, or a state with no rows.
 * Best row.  best[i] (int32) is the lowest row number k of the state with c(row_off[i] + k) == cost[i] - 1; -1 at goal states
 * and dead ends.
 * Row bits.  Row r of state i is optimal iff cost[i] > 0 and c(r) == cost[i] - 1.  It is safe iff c(r) is finite.
 * info (int64 [5]): states, rows, goal states (cost == 0), dead ends, largest finite cost (-1 when no state has one).
 * A cost in moves is left out on purpose: the store keeps ONE agent position per canonical state, so a cost in moves is not a
 * function of the node (as K15's plans over pushes minimise pushes, not moves).  The push set of a state is a function of its
 * canonical state -- the same region and the same boxes give the same rows in the same order -- so the rows stored for node i
 * are the rows of any live state that maps to node i; only the walk distances differ.  The query relies on this.
 *
 * pw_push_search_solve is synchronous.  PW_EINVAL naming the condition: a null handle or info; a call before
 * pw_push_search_begin; stop_at_goal set; layers left to expand; an overflowed store.  PW_ELIMIT when R > 2^31 - 1.
 * pw_push_search_begin and pw_push_search_destroy discard the table.
 *   successor pass  one pass per PW_OPT_SEARCH_CHUNK parents over the whole store, exactly the front half of a pass of
 *                   pw_push_search_expand (the counts out of the store, the scan, the rows flood, the regions flood of the
 *                   successors, the candidates) in the search's own workspace, grown as pw_push_search_expand grows it; the
 *                   host waits once per pass, for the row count.  A read-only lookup then probes the closed set from the
 *                   candidate's first slot and accepts a published entry only when the fingerprint matches and the packed
 *                   canonical state equals the store's words: exact under PW_OPT_PUSH_SEARCH_FP_BITS.  The closed set is never written.
 *   sweeps          level-synchronous: sweep d gives cost d to every state that is still unset and has a row with c == d - 1,
 *                   and records the lowest such row.  A sweep after one that changed nothing changes nothing, so 8 sweeps are
 *                   queued per host read of their changed-counters; the sweeps end at the first that changed nothing and never
 *                   run more than S times.  A last row pass writes the optimal and safe bits.
 * Device memory: 16 bytes per state (row_off, cost, best) and 8 bytes per row (succ, from, action, flags) of the table; during
 * pw_push_search_solve 4 more bytes per row (the row -> state map of the sweeps) and 64 bytes of counters, freed when it returns.
 * No kernel waits on another workgroup; every loop is bounded by the rows, the slots, S or the 4 095 steps of a walk. */
int  pw_push_search_solve(PwPushSearch* s, int64_t info[5], void* stream);
/* states first .. first + count - 1 (row_off: count + 1 values, absolute row numbers) / rows first .. first + count - 1 into device
   buffers, any of which may be NULL; asynchronous on `stream`.  PW_EINVAL: a null handle, a range outside the table, no table. */
int  pw_push_search_table_read(PwPushSearch* s, int64_t first_state, int64_t count, int64_t* row_off /* [count + 1] */,
                               int32_t* cost, int32_t* best, void* stream);
int  pw_push_search_table_rows(PwPushSearch* s, int64_t first_row, int64_t count, int32_t* succ, int8_t* from, uint8_t* action,
                               uint8_t* flags, void* stream);
/* Live states -> table rows and the expert's next action.  puzzle_id / pos / npad / mask and the conventions are
 * pw_search_table_query's: puzzle_id device int32 [n] or NULL (every item is of the table's puzzle), pos device int8 [n][npad][2],
 * mask device uint8 [n] or NULL (0 skips an item).  Items of other puzzles and masked items are LEFT UNTOUCHED: several tables fill
 * one set of outputs for a mixed batch.  For every other item (all outputs are device pointers, any may be NULL):
 *   index[i]       int32     the store index; -1 when the state is not in the table or a coordinate is outside the grid
 *   cost[i]        int32     pushes to go; -1 at a dead end; -2 when the state is not in the table
 *   push_from[i]   int8 [2], push_action[i] uint8: the state's best row, out of the table's rows; (0, 0) and 0xFF when there is none
 *   walk[i]        int32     dist(push_from) in the LIVE state's walk map; -1 when there is none
 *   action[i]      int8      the first primitive action of "walk to push_from, then push": push_action when walk == 0, else the
 *                            parent action of the position at distance 1 on the way back from push_from along the map's parent
 *                            actions; -1 when there is none (goal, dead end, not in the table)
 * One small kernel forms the effective mask (mask && id == puzzle), one regions flood runs over the items that take part (the
 * walk maps are made only when walk or action is asked for), and one kernel with one lane per item applies the lookup of the
 * successor pass to the live state's own packed canonical state and writes the outputs.
 * The workspace -- the maps, 2 * map_h * map_w bytes per item at the set's largest dimensions, and 19 bytes of per-item words --
 * belongs to the handle; it is allocated on first use or growth and synchronises `stream` then.  Otherwise the call is
 * asynchronous, reads nothing on the host and is capturable.  ONE query at a time per handle.
 * PW_EINVAL before any launch, pw_last_error naming the function: a null handle, n < 1, a null pos, npad not 4 / 8 / 16 / 32 or
 * smaller than the set's largest number of movables, no solved table. */
int  pw_push_search_table_query(PwPushSearch* s, const int32_t* puzzle_id, const int8_t* pos, int32_t npad,
                                const uint8_t* mask, int32_t n, int32_t* index, int32_t* cost, int8_t* push_from,
                                uint8_t* push_action, int32_t* walk, int8_t* action, void* stream);

/* Drawing from a table over pushes (K20): K14's cost index, sample and plans for the table of pw_push_search_solve, and an
 * emit that turns plans into flat demonstration rows.  All work on a PwPushSearch that holds a solved table; S is its number
 * of states and mc = info[4] its largest finite cost (-1: none).  The streams are K14's: mix64 is pw_mix64,
 * PW_TABLE_K_SAMPLE = 0xA0761D6478BD642F, PW_TABLE_K_PLAN = 0xE7037ED1A0B428DB.
 *
 * ..._index: builds the cost index over STATES (a state has several rows) unless the handle has it (idempotent):
 *     states_by_cost  int32 [S]        a permutation of the store indices: all states of cost 0, then cost 1, ... mc, then the
 *                                      dead ends (cost -1) as the last bucket; INSIDE A BUCKET IN ASCENDING STORE INDEX
 *     cost_start      uint32 [mc + 3]  bucket c is [cost_start[c], cost_start[c + 1]); the dead ends are bucket mc + 1; the
 *                                      last entry is S.  mc == -1: the two words [0, S].  A bucket may be empty: a table whose
 *                                      goal rows all leave the grid has no state of cost 0.
 *   K16's numbering of the store is deterministic, so with the order inside a bucket fixed a draw is a pure function of
 *   (puzzle, start, seed, environment, count), whatever the build or the schedule.  One kernel writes (bucket, store index) per
 *   state and counts the buckets, one stable rocPRIM radix sort by bucket orders the states, one scan makes cost_start.  The
 *   call allocates (4 bytes per state and per bucket, kept; 12 bytes per state and the sort's workspace, freed on return) and
 *   synchronises `stream` once.  pw_push_search_begin, a new pw_push_search_solve and pw_push_search_destroy discard the index.
 * ..._index_read: the two arrays copied into caller device buffers (either may be NULL), asynchronous on `stream`.
 *
 * ..._sample: pw_search_table_sample's arguments and semantics, with out_state (the store index drawn) in place of out_row.
 *   ONE launch, no allocation, no synchronisation (capturable), one thread per environment; the index must exist.  Masked
 *   environments, and environments of another puzzle when puzzle_id is not NULL, are LEFT ENTIRELY UNTOUCHED, the counter
 *   included.  The band -- the scalars lo, hi, or lo_n / hi_n per environment with hi < lo read as hi = lo -- is clamped to
 *   [0, mc]; dead ends are never drawn.  A table with no finite cost, and a band that holds no state (cost 0 in a table without
 *   goal states in its store), give out_state = out_cost = -1 and nothing else is written.  Else
 *     counter[i] += 1;  r = mix64(seed ^ PW_TABLE_K_SAMPLE, i, counter[i])
 *     count = cost_start[hi + 1] - cost_start[lo];  u = floor(r * count / 2^64);  state = states_by_cost[cost_start[lo] + u]
 *   and the environment is written as pw_reset writes it: pos = the store's state AS REACHED (zeros from the puzzle's N to
 *   npad - 1), steps = 0, term = trunc = 0 (either may be NULL); out_state = state, out_cost = its cost.  npad is 4 / 8 / 16 /
 *   32 and at least the puzzle's number of movables.  Every agent position of the node's walk region is the same node; only
 *   the stored one is drawn.
 *
 * ..._plans: ONE launch (capturable, no index needed), one thread per item: the walk from store index index[i] (as the query
 *   returns it) down to cost 0.
 *     plan_from    device int8 [n][plan_cap][2]     plan_action  device uint8 [n][plan_cap]
 *     plan_state   device int32 [n][plan_cap] or NULL: the node the t-th push is made from
 *     plan_len     device int32 [n]
 *   At state i with cost > 0, tie 0 takes row row_off[i] + best[i]; tie 1 takes, at step t, the j-th optimal row (flags bit 1)
 *   of the state in row order, with k the number of its optimal rows and j = floor(mix64(seed ^ PW_TABLE_K_PLAN, item, t) * k
 *   / 2^64).  A goal row (flags bit 0) ends the plan, whatever its succ is; otherwise the walk goes on to succ (an optimal row
 *   is safe: never -1).  plan_len is the start's cost when 0 <= cost <= plan_cap; -1 for an index outside [0, S), a dead end
 *   or an item of another puzzle (the plan arrays untouched); -2 when the cost exceeds plan_cap (nothing is written).  Masked
 *   items are untouched.
 *
 * ..._emit: ONE launch (capturable), one thread per (item, step): push t of the plan of item i becomes row offset[i] + t.
 *     pos      device int8 [n][npad][2]: the items' live states, or NULL: the stored state of plan_state[i][0]
 *     offset   device int64 [n + 1]: the exclusive scan of max(plan_len, 0) over the items that take part, made by the caller
 *     row_item, row_t, row_state, row_cost  device int32 [rows_cap]     row_from  int8 [rows_cap][2]     row_action  uint8 [rows_cap]
 *     row_pos  device int8 [rows_cap][npad][2]                          dropped   device uint32 [1], added to
 *   row_state = plan_state[i][t], row_from / row_action the t-th push, row_cost = plan_len[i] - t.  row_pos of t = 0 is the
 *   live state (or the stored one); for t > 0 it is the movables of the store's state plan_state[i][t] with the agent's pair
 *   replaced by plan_from[i][t - 1] plus the displacement of plan_action[i][t - 1] (0 left, 1 right, 2 up, 3 down).  No flood
 *   and no step function: a node's key is its canonical state, so the successor's boxes are the store's, and a push move
 *   displaces its push set, the agent included, by exactly one cell.  State words go out with 8-byte (npad 4) or 16-byte
 *   stores.  Rows at or beyond rows_cap (and rows whose plan_state lies outside the store) are dropped and counted into
 *   `dropped`.  Items of other puzzles, masked items and items with plan_len <= 0 write nothing.
 *
 * PW_EINVAL before any launch, pw_last_error naming the function: a null handle or a null required array; n < 1; npad not 4 / 8
 * / 16 / 32 or smaller than the puzzle's number of movables; band arrays that do not come together, or scalars without
 * 0 <= lo <= hi; plan_cap < 1; tie not 0 / 1; rows_cap < 0; no solved table; sample without an index.  No kernel waits on
 * another workgroup; there is no device assert; every loop is bounded by the items, a state's rows, plan_cap or the start's cost. */
int  pw_push_search_table_index(PwPushSearch* s, void* stream);
int  pw_push_search_table_index_read(PwPushSearch* s, int32_t* states_by_cost, uint32_t* cost_start, void* stream);
int  pw_push_search_table_sample(PwPushSearch* s, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                                 uint64_t seed, uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n,
                                 const int32_t* hi_n, int8_t* pos, int32_t* steps, uint8_t* term, uint8_t* trunc,
                                 int32_t* out_state, int32_t* out_cost, void* stream);
int  pw_push_search_table_plans(PwPushSearch* s, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                                int32_t tie, uint64_t seed, int8_t* plan_from, uint8_t* plan_action, int32_t* plan_state,
                                int32_t plan_cap, int32_t* plan_len, void* stream);
int  pw_push_search_table_emit(PwPushSearch* s, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                               const int8_t* plan_from, const uint8_t* plan_action, const int32_t* plan_state, int32_t plan_cap,
                               const int32_t* plan_len, const int8_t* pos, const int64_t* offset, int64_t rows_cap,
                               int32_t* row_item, int32_t* row_t, int32_t* row_state, int8_t* row_from, uint8_t* row_action,
                               int32_t* row_cost, int8_t* row_pos, uint32_t* dropped, void* stream);

/* Best-first search over pushes (K17): K16's nodes, store, closed set and links, expanded in the order of the reference's RGD
 * heuristic instead of layer by layer.  A node is a canonical state; the store keeps the state as reached and its canon; state 0
 * is the start; the fields per state are K16's (pos, canon, parent, from, action, walk, goal, region size, push count).
 * Key: the RGD cost in fewest-tools mode (the reference default) of the state as reached -- the agent stands where the push
 * left it -- from pw_rgd_* with the handle's budget.  The queue is pw_planner's: integer buckets for finite costs (range 2^22),
 * then +inf, then NaN (a budget overrun, or a movable off its movement graph).  A finite cost beyond the range ends the run with
 * PW_ELIMIT; it is never clamped.  Within a bucket the newest entry pops first; the states of one round enter in store order,
 * so the highest store index pops first.  +inf and NaN states are pushed and popped last, so that "exhausted" means exhausted.
 * Begin: a start that is a goal state is solved at once (goal index 0, empty plan, nothing pushed).  Otherwise the start is
 * flooded and published as state 0, as pw_push_search_begin does, and pushed under its key.
 * A round, in this order:
 *   1 pop     an empty queue: status PW_PLAN_EXHAUSTED.  Otherwise up to K states, lowest bucket first; rounds += 1, expanded +=
 *             the number popped, open -= the number popped.
 *   2 count   T = the sum of the popped states' stored push counts; push rows += T.
 *   3 limit   states + T > max_states: status PW_PLAN_LIMIT; nothing is appended and the counters keep what 1 and 2 did
 *             (conservative and deterministic, as pw_planner's stored + 4 K).
 *   4 rows    the push moves of the popped states in pop order, a state's in pw_walk_pushes' (y, x, action) order.
 *   5 append  a successor is appended when it lies inside its grid, its canonical state is not closed, and it is the first row
 *             in that order with that canonical state (the lowest row owns it: K16's atomicMin rule, so the numbering does not
 *             depend on which workgroup ran first).
 *   6 goal    the successor of the first row (in that order) into a goal state is the last state of the store, published even
 *             if it owns no entry of the closed set (K16's stop_at_goal rule, its out-of-grid goal row included); status
 *             PW_PLAN_SOLVED, goal index = states - 1; nothing is pushed in that round.
 *   7 push    otherwise every new state is evaluated and pushed in store order; largest region takes the maximum of the new
 *             states' region sizes.
 * The plan is pw_push_search_plan's: the chain of parents (bounded by the number of states, not by a depth), the walks between
 * pushes taken from the parent actions of the walk maps.
 * pw_push_planner_run runs at most max_rounds rounds (<= 0: to the end) and waits once per round: it reads the status and T
 * together, grows the row workspace if T asks for it, and enqueues the rest of the round.  After an end (solved, exhausted,
 * limit) it returns the same info again; pw_push_planner_begin starts afresh.
 *   info[0] status (PW_PLAN_RUNNING, PW_PLAN_SOLVED, PW_PLAN_EXHAUSTED, PW_PLAN_LIMIT)
 *   info[1] rounds           info[2] expanded         info[3] states in the store    info[4] open
 *   info[5] goal index, or -1                         info[6] RGD budget overruns since begin
 *   info[7] push rows        info[8] largest region   info[9] largest finite key pushed, or -1
 * Device memory: K16's per state and per row, 16 bytes of queue per state of max_states, 16 MiB of bucket heads, and per push
 * row of the largest round 4 N + 20 bytes of keys.  PW_OPT_PUSH_SEARCH_FP_BITS applies as in K16.
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: a null handle, engine, out or info;
 * max_states outside 1 .. 2^31 - 1; batch outside 1 .. 65 536; a negative rgd_budget; a puzzle index outside the set; a start
 * with a movable outside its grid; a range outside the store; run, plan or a read before begin; plan when the search is not
 * solved. */
typedef struct PwPushPlanner PwPushPlanner;
int  pw_push_planner_create(PwEngine* e, int32_t puzzle, int64_t max_states, int32_t batch /* K, 1 .. 65536 */,
                            int64_t rgd_budget /* 0 = default */, PwPushPlanner** out);
void pw_push_planner_destroy(PwPushPlanner* p);
/* start: host int8 [N][2] (x, y) or NULL = the initial state.  Synchronises. */
int  pw_push_planner_begin(PwPushPlanner* p, const int8_t* start, void* stream);
int  pw_push_planner_run(PwPushPlanner* p, int64_t max_rounds /* <= 0: to the end */, int64_t info[10], void* stream);
/* as pw_push_search_read_states / pw_push_search_read_links, over the states counted by the last run (1 after begin) */
int  pw_push_planner_read_states(PwPushPlanner* p, int64_t first, int64_t count, int8_t* pos, int8_t* canon, void* stream);
int  pw_push_planner_read_links(PwPushPlanner* p, int64_t first, int64_t count, int32_t* parent, int8_t* from,
                                uint8_t* action, int32_t* walk, uint8_t* goal, void* stream);
/* The plan to the goal state, as pw_push_search_plan (host buffer; returns the length, nothing written if > cap). */
int  pw_push_planner_plan(PwPushPlanner* p, uint8_t* actions, int32_t cap, int32_t* pushes, void* stream);

/* Exact cost-to-go tables OVER PUSHES (pw_push_search_solve's definitions: canonical states, push rows in (y, x, action) order,
 * succ / cost / best / flags) of MANY small puzzles in ONE launch (csrc/pw_push_solution_batch.inc), in the form of
 * pw_solve_batch: persistent workgroups take items off a device counter and do the search over canonical states, the rows, the
 * sweeps (a barrier each) and the row bits of an item inside the kernel.  The walk regions are flooded on the packed state word
 * with the step pw_solve_batch_run takes, the agent's byte replaced, so the definitions are those of pw_walk_regions / pw_walk_pushes:
 * (q, a) is a walk move when stepping the state with the agent at q moves the agent and nothing else, a push move when it moves
 * the agent and at least one other movable; a position at which the agent's bounding box leaves the grid is not in the region;
 * canon is the region's smallest position in (y, x) order.  A node's key is the packed word (movable j at bits 8 j, x in the low
 * nibble, y in the high one) with the agent at canon and zeros beyond the puzzle's N.
 * Limits: 16 x 16 cells with the border, at most 8 movables, overlap tables present; anything else gets status 3.
 *
 * pw_push_solve_batch_create: states_cap, rows_cap >= 0: the pools for the tables of all items together (0 / 0: summaries only).
 *   A stored item takes its states + 1 entries of the state pool and its rows of the row pool.
 * pw_push_solve_batch_run: `puzzles` device int32 [n] set indices or NULL = 0 .. n - 1; `starts` device int8 [n][npad][2] (npad
 *   4 / 8 / 16 / 32, at least the set's movables; only the first N movables of a row are read) or NULL = each puzzle's initial
 *   state; a start outside its grid gives status 3.  Asynchronous on `stream` except when the engine's slabs or the handle's
 *   per-item arrays have to grow.
 * Per item, in device arrays owned by the handle (pw_push_solve_batch_results; valid until the next run or the destroy):
 *   status     uint8      0 built and stored   2 more than max_states_each states (or more than 32 x max_states_each rows)
 *                         3 not searched   4 built, but a pool was full: the summary is valid, nothing is stored
 *                         5 a finite cost reached 65 535   6 a successor was missing from the exhausted closed set (internal)
 *   summary    int32 [6]  states, rows, goal states, dead ends, largest finite cost (-1: none), cost of the start (-1: a dead
 *                         end); valid for status 0 and 4 (else: states and rows found so far, then 0 0 -1 -1)
 *   state_off / row_off   int64: the item's first entry in the state pool / the row pool, -1 when it is not stored
 * State 0 is the start, and the order of a state's rows, best, the costs and the bits are fixed.  State numbers inside a layer,
 * hence succ, and the pool offsets depend on the schedule and may differ from run to run: everything is found by state.
 * pw_push_solve_batch_totals (synchronises `stream`): [0] the state-pool entries and [1] the rows that store every built table
 *   of the run (size a second handle with them), [2] lookup slots in use, [3] missing successors (0).
 * pw_push_solve_batch_read_states: states first .. first + count - 1 of a stored item into device buffers (any may be NULL):
 *   key uint64, row_off int64 [count + 1] (first row of each state, relative to the item's first row), cost int32 (-1: a dead
 *   end), best int32 (the lowest row of the least value, relative to the state's first; -1 at goal states and dead ends).
 * pw_push_solve_batch_read_rows: rows first .. first + count - 1 of a stored item: succ int32 (state within the item, -1: the
 *   successor lies outside the grid), from int8 [2], action uint8, flags uint8 (bit 0 goal row, 1 optimal, 2 safe).
 *   The first read after a run fetches the item offsets (synchronises `stream` once); asynchronous afterwards.
 * pw_push_solve_batch_query: live states of a MIXED batch, ONE launch, no allocation, no synchronisation (capturable): per item
 *   the lookup of its puzzle's item, the range check and packing of the first N movables, the flood of the live region (a
 *   layered breadth-first search that keeps a 2-bit parent action per cell when walk or action is asked for), the probe of the
 *   canonical key confirmed against the stored key, and the way back from push_from along the parents.  Outputs and conventions
 *   are exactly pw_push_search_table_query's (index, cost -1 dead end / -2 not in the table, push_from, push_action 0xFF, walk,
 *   action; any may be NULL).  Masked items and items whose puzzle has no STORED table in this handle are LEFT UNTOUCHED.
 *   A puzzle listed twice is answered from its higher item.
 * Every argument check returns PW_EINVAL before any launch and names the function (null handle, n < 1, null puzzle_id / pos,
 * npad not 4 / 8 / 16 / 32 or below the set's movables, negative caps, no run yet).
 * Memory: 24 bytes per entry of the state pool (8 key + 8 row_off + 4 cost + 4 best), 8 bytes per row (4 succ + 2 from +
 * 1 action + 1 flags), 4 bytes per lookup slot -- a power of two >= 2 x states (at least 16) slots per stored item, reserved as
 * 4 slots per state + 16 per item; 50 bytes per item; 4 bytes per puzzle of the set.  The engine's slabs (shared with
 * pw_search_batch, PW_OPT_SEARCH_BATCH_GROUPS_PER_CU applies): per persistent workgroup 400 bytes per state of max_states_each
 * (16 per state + 32 rows of 12 bytes) + 12 bytes per slot of the 2^16 / 2^20 / ... closed-set levels. */
typedef struct PwPushSolveBatch PwPushSolveBatch;
int pw_push_solve_batch_create(PwEngine* e, int64_t states_cap, int64_t rows_cap, PwPushSolveBatch** out);
void pw_push_solve_batch_destroy(PwPushSolveBatch* b);
int pw_push_solve_batch_run(PwPushSolveBatch* b, const int32_t* puzzles, const int8_t* starts, int32_t npad, int32_t n,
                            int64_t max_states_each, void* stream);
/* device pointers (any may be NULL); returns the number of items of the last run */
int pw_push_solve_batch_results(PwPushSolveBatch* b, const uint8_t** status, const int32_t** summary, const int64_t** state_off,
                                const int64_t** row_off);
/* the same arrays copied into the caller's device buffers [n], [n][6], [n], [n] (any may be NULL), asynchronous on `stream` */
int pw_push_solve_batch_copy_results(PwPushSolveBatch* b, uint8_t* status, int32_t* summary, int64_t* state_off, int64_t* row_off,
                                     void* stream);
int pw_push_solve_batch_totals(PwPushSolveBatch* b, int64_t totals[4], void* stream);
int pw_push_solve_batch_read_states(PwPushSolveBatch* b, int32_t item, int64_t first, int64_t count, uint64_t* key,
                                    int64_t* row_off, int32_t* cost, int32_t* best, void* stream);
int pw_push_solve_batch_read_rows(PwPushSolveBatch* b, int32_t item, int64_t first, int64_t count, int32_t* succ, int8_t* from,
                                  uint8_t* action, uint8_t* flags, void* stream);
int pw_push_solve_batch_query(PwPushSolveBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                              int32_t n, int32_t* index, int32_t* cost, int8_t* push_from, uint8_t* push_action, int32_t* walk,
                              int8_t* action, void* stream);

/* Drawing from the batched tables over pushes (csrc/pw_push_batch_sample.inc, K26): pw_push_search_table_index / _sample / _plans
 * / _emit for a PwPushSolveBatch whose last run stored tables -- the cost index of every stored item, and ONE launch per call for
 * a mixed batch however many puzzles it holds.  A node's key is its canonical state, so states are read off the keys.
 *
 * pw_push_solve_batch_index: the cost index of every stored item, built on demand, idempotent; the next pw_push_solve_batch_run
 *   and the destroy discard it.  Per stored item with S states and largest finite cost mc:
 *     states_by_cost int32 [S]       a permutation of the item's state numbers: cost 0, 1, ... mc, then the dead ends
 *     cost_start     uint32 [mc + 3] bucket c = states_by_cost[cost_start[c] .. cost_start[c + 1]), the dead ends are bucket
 *                                    mc + 1, cost_start[mc + 2] = S; mc = -1: [0, S].  Empty buckets occur (a store without goal
 *                                    states has no state of cost 0).
 *   Inside a bucket the states ascend by their 64-BIT KEY: state numbers inside a layer are the schedule's, the key is not, so
 *   position p of a bucket holds the same STATE in every run and a draw is a function of (puzzle, start, seed, environment,
 *   count) as a state.  Allocates (4 bytes per stored state and per bucket, 16 per item; a workspace of 32 bytes per state
 *   plus the sorts' own is freed on return) and synchronises `stream`.
 * pw_push_solve_batch_index_read: one item's two arrays into device buffers (either may be NULL), asynchronous.
 * pw_push_solve_batch_sample: pw_push_search_table_sample's arguments and semantics with puzzle_id required; one thread per
 *   environment, no allocation, no synchronisation (capturable).  The item is the one pw_push_solve_batch_query answers from
 *   (a puzzle listed twice: its higher item).  Masked environments and environments whose puzzle has no stored item are left
 *   ENTIRELY untouched, the counter included.  The band is clamped to 0 .. mc of the environment's own item, dead ends are never
 *   drawn; an item without a finite cost or an empty band gives out_state = out_cost = -1, nothing else written, the counter
 *   not advanced.  Otherwise counter[i] += 1, r = mix64(seed ^ PW_TABLE_K_SAMPLE, i, counter[i]), u = floor(r * count / 2^64),
 *   the state is states_by_cost[cost_start[lo] + u]: pos[i] = its key unpacked (the agent at canon, zeros from the puzzle's N
 *   to npad - 1; 8- or 16-byte stores), steps = 0, term = trunc = 0 (either may be NULL), out_state = the state within the item
 *   (what pw_push_solve_batch_query returns for it), out_cost = its cost.
 * pw_push_solve_batch_plans: pw_push_search_table_plans' arguments with puzzle_id required; no index needed; one thread per
 *   item.  tie 0: row row_off[state] + best[state]; tie 1: the j-th optimal row in row order, j = floor(mix64(seed ^
 *   PW_TABLE_K_PLAN, item, t) * k / 2^64) of k.  A goal row ends the plan whatever its succ.  plan_len = the cost; -1 for an
 *   index outside the item, a dead end or a puzzle without a stored item; -2 for a cost beyond plan_cap (nothing else written).
 * pw_push_solve_batch_emit: pw_push_search_table_emit's arguments with puzzle_id required; one thread per (item, step).  Row
 *   offset[i] + t: row_item, row_t, row_state (within the item), row_from, row_action, row_cost = plan_len - t, and row_pos --
 *   for t = 0 pos[i] (pos NULL: the unpacked key of plan_state[i][0]), for t > 0 the movables of the key of plan_state[i][t]
 *   with the agent's pair replaced by plan_from[i][t - 1] displaced by plan_action[i][t - 1].  Rows at or beyond rows_cap and
 *   rows whose plan_state lies outside the item are counted into `dropped`; items of puzzles without a stored item are skipped.
 * Argument checks (PW_EINVAL before any launch, naming the function): those of the pw_push_search_table_* calls, null
 * puzzle_id, no run yet, nothing stored (pools of size 0, or no stored item), sample / index_read without an index, npad below
 * the set's movables. */
int pw_push_solve_batch_index(PwPushSolveBatch* b, void* stream);
int pw_push_solve_batch_index_read(PwPushSolveBatch* b, int32_t item, int32_t* states_by_cost, uint32_t* cost_start, void* stream);
int pw_push_solve_batch_sample(PwPushSolveBatch* b, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                               uint64_t seed, uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n,
                               int8_t* pos, int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_state, int32_t* out_cost,
                               void* stream);
int pw_push_solve_batch_plans(PwPushSolveBatch* b, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                              int32_t tie, uint64_t seed, int8_t* plan_from, uint8_t* plan_action, int32_t* plan_state,
                              int32_t plan_cap, int32_t* plan_len, void* stream);
int pw_push_solve_batch_emit(PwPushSolveBatch* b, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                             const int8_t* plan_from, const uint8_t* plan_action, const int32_t* plan_state, int32_t plan_cap,
                             const int32_t* plan_len, const int8_t* pos, const int64_t* offset, int64_t rows_cap,
                             int32_t* row_item, int32_t* row_t, int32_t* row_state, int8_t* row_from, uint8_t* row_action,
                             int32_t* row_cost, int8_t* row_pos, uint32_t* dropped, void* stream);

/* Best-first search over pushes (pw_push_planner_*, K17) of MANY puzzles or live states in ONE launch
 * (csrc/pw_push_plan_batch.inc, K24), in the form of pw_plan_batch: persistent workgroups of one wavefront take items off a
 * device counter and run the whole search of an item -- pop, the floods, the push rows, the closed set, the goal test, RGD, push
 * -- inside the kernel.  Item i's info[0..9], store (the states as reached and their canon) and links (parent, from, action,
 * goal) equal pw_push_planner_create(e, puzzle, max_states, batch, rgd_budget) + begin(start) + run(max_rounds), round by round
 * (the seven steps listed there), as long as no finite key reaches cost_range.  The walk regions are flooded on the packed state
 * word as pw_push_solve_batch does, so the limits are its limits: 16 x 16 cells with the border, at most 8 movables, overlap
 * tables present, the start inside its grid.  An item beyond them is PW_PLAN_SKIPPED: info[0] = 6, info[1..10] = 0, plan_len -1,
 * first_from (0, 0), first_action PW_PUSH_NONE; nothing of it is read past the test that skips it.
 *
 * pw_push_plan_batch_create: `puzzles` host int32 [n] set indices or NULL = 0 .. n - 1; batch = K, 1 .. 64; max_states per item,
 *   1 .. 2^28; rgd_budget 0 = the default; cost_range 1 .. 65536 finite keys with a bucket (0 = 65536): a finite key at or
 *   above it ends that item with PW_PLAN_RANGE.  Builds the RGD tables of every listed puzzle within the limits and the
 *   workgroups' slabs: at most two per CU, one per item, within a quarter of the free memory.  Per state of max_states a slab
 *   holds 21 bytes (key 8, agent byte 1, parent 4, from 2, action 1, goal 1, next 4) and 16 to 32 bytes of the closed set
 *   (tag << 32 | index + 1, a power of two >= 2 max_states slots), plus 4 bytes per bucket.
 * pw_push_plan_batch_run: item i is listed puzzle i from its initial state.  Asynchronous on `stream`: a one-thread kernel that
 *   zeroes the item counter and takes n fresh closed-set tags from a counter ON THE DEVICE, then the search kernel; no allocation,
 *   no wait, nothing read on the host.  Capturable, and a captured call may be replayed any number of times: every replay takes
 *   its own tags, so it never meets the closed-set entries of the replay before, and it plans from whatever the inputs hold then.
 *   max_rounds per item (<= 0: no limit); time_limit seconds per item on the device's constant clock (0 = none; an item past it
 *   ends with PW_PLAN_TIMEOUT; checked between rounds); pw_push_plan_batch_cancel stops every eager launch made so far, queued
 *   ones included, and every replay of a captured launch that has begun, within 32 rounds per item (status PW_PLAN_RUNNING with
 *   the counts reached; items not started: 0 rounds, goal index -1).  A replay that begins after the cancel runs as usual: a
 *   captured launch carries no sequence number, it compares the cancel generation it found when it began.
 *   All outputs are device memory; any but info may be NULL:
 *     info         int64 [n][PW_PUSH_PLAN_BATCH_INFO]: pw_push_planner_run's ten values, then the item's search time in ns
 *     plan_len     int32 [n]: the number of pushes of the plan; -1 no plan; -2 the plan is longer than push_cap and nothing of
 *                  it is written (only with plan arrays); 0 the start is a goal state
 *     plan_from    int8 [n][push_cap][2], plan_action uint8 [n][push_cap]: the chain of parents written forwards
 *     plan_pos     int8 [n][push_cap][npad][2]: the state as reached that push t is made from, zeros beyond N -- the rows that
 *                  pw_push_unroll_count / _write take.  Entries at and past plan_len are left as they are.
 * pw_push_plan_batch_run_states: item i is the state pos[i] (device int8 [n][npad][2], the engine's layout) of puzzle
 *   puzzle_id[i] (device int32 [n]); mask device uint8 [n] or NULL, 0 = skip.  Items that are masked out, name a puzzle outside
 *   the set or one the handle did not prepare, or hold a movable outside its grid are PW_PLAN_SKIPPED.  first_from int8 [n][2]
 *   and first_action uint8 [n]: the first push of a plan with plan_len > 0, else (0, 0) and PW_PUSH_NONE; either way
 *   pw_step_push takes them as they are.  The same two kernels, capturable and replayable once the workgroups exist: a call with more
 *   items than workgroups (below two per CU) replaces the slabs first and waits for the device once, as pw_plan_batch_run_states
 *   does -- make one eager call with the batch size before capturing.
 * pw_push_plan_batch_read_states / _read_links: the store of `item` of the last launch into device buffers (any may be NULL):
 *   pos int8 [count][npad][2] and canon int8 [count][2]; parent int32, from int8 [count][2], action uint8 (PW_PUSH_NONE for the
 *   start), goal uint8.  A workgroup keeps the store of the LAST item it ran: every item of a launch with n <= the number of
 *   workgroups can be read, of a larger launch those that no later item displaced; a displaced or skipped item is PW_EINVAL.
 *   Synchronises `stream` once per call.
 * PW_EINVAL before any launch, pw_last_error naming the function and the argument: a null engine, out, handle, puzzle_id, pos
 * or info; n < 1; batch outside 1 .. 64; max_states outside 1 .. 2^28; a negative rgd_budget; cost_range outside 0 .. 65536; a
 * negative time_limit; npad not 4 / 8 / 16 / 32 or below the prepared movables; push_cap < 0; plan arrays without plan_len; a
 * puzzle index outside the set; a read before a run, of a range outside the store or of an item whose store is gone. */
#define PW_PUSH_PLAN_BATCH_INFO 11
#define PW_PUSH_NONE 0xFF
typedef struct PwPushPlanBatch PwPushPlanBatch;
int pw_push_plan_batch_create(PwEngine* e, const int32_t* puzzles, int32_t n, int64_t max_states, int32_t batch,
                              int64_t rgd_budget, int32_t cost_range, PwPushPlanBatch** out);
int pw_push_plan_batch_run(PwPushPlanBatch* b, int64_t max_rounds, double time_limit, int64_t* info, int32_t* plan_len,
                           int8_t* plan_from, uint8_t* plan_action, int8_t* plan_pos, int32_t push_cap, int32_t npad,
                           void* stream);
int pw_push_plan_batch_run_states(PwPushPlanBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad,
                                  const uint8_t* mask, int32_t n, int64_t max_rounds, double time_limit, int64_t* info,
                                  int32_t* plan_len, int8_t* plan_from, uint8_t* plan_action, int8_t* plan_pos, int32_t push_cap,
                                  int8_t* first_from, uint8_t* first_action, void* stream);
int pw_push_plan_batch_read_states(PwPushPlanBatch* b, int32_t item, int64_t first, int64_t count, int8_t* pos, int32_t npad,
                                   int8_t* canon, void* stream);
int pw_push_plan_batch_read_links(PwPushPlanBatch* b, int32_t item, int64_t first, int64_t count, int32_t* parent, int8_t* from,
                                  uint8_t* action, uint8_t* goal, void* stream);
int pw_push_plan_batch_cancel(PwPushPlanBatch* b);
void pw_push_plan_batch_destroy(PwPushPlanBatch* b);

/* Cost-to-go guidance inside the step (csrc/pw_guide.inc, K28): ONE launch behind a step launch (and behind pw_start_pool_draw,
 * in front of pw_episode_stats) leaves per environment the exact cost-to-go of the state the step left, its optimal / safe
 * action bits, whether it is a dead end and the potential-shaped reward; it counts guided / optimal / dead-entering / unknown
 * steps per puzzle and, asked to, truncates an environment that has just entered a dead end.  One lane per environment, no
 * allocation, no synchronisation, capturable.  The integers are exact and independent of launch geometry and atomic order; the
 * shaped reward is made of individually rounded double operations (no fused multiply-add), so it is too.  Every argument error
 * returns PW_EINVAL with the function's name and the offending argument in pw_last_error, before anything is read through a
 * pointer.
 *
 * The source of the lookup -- exactly one of:
 *   tables   a PwSolveBatch of this engine with a run (the fused form): the kernel looks (puzzle_id[i], pos[i]) up itself.  Its
 *            answer (c, a) is pw_solve_batch_query's cost and acts -- the first N movables of the row only, -2 / 0 for a movable
 *            outside 0 .. 15 or outside the grid and for a state the table does not hold, -1 for a dead end -- and -2 / 0 also
 *            for a puzzle without a stored table and for an id outside 0 .. P - 1.
 *   cost_in  device int32 [n], with acts_in device uint8 [n] or NULL (the applied form): (c, a) = (cost_in[i], acts_in[i] or 0),
 *            what the query launches of any table kind wrote into buffers that held -2 / 0.  The kernel stores cost_in[i] = -2
 *            and acts_in[i] = 0 behind its read, so that the next call's queries start clean.
 * Environment state: puzzle_id int32 [n], pos int8 [n][npad][2], reward double [n] (read only, may be NULL without shaped),
 * terminated uint8 [n] (read only), truncated uint8 [n] (read and written), mask uint8 [n] or NULL.
 * Guide state, [n] each: cost int32 (in / out), acts uint8 (out), seen uint8 (in / out: the environment's flags as the previous
 * guide call left them), dead uint8 (out), shaped double (out, may be NULL).
 * Parameters: dead_cost int32 [P] (may be NULL without shaped), gamma, scale, counts int64 [P][PW_GUIDE_COUNTS] (may be NULL).
 *
 * The rule for environment i < n, with p = puzzle_id[i] and (c, a) the lookup of the state as the step left it:
 *   0. mask != NULL and mask[i] == 0: nothing is written for i at all (cost_in / acts_in included).
 *   1. PW_GUIDE_REFRESH (behind a reset or anything else that moved the environment outside a step): cost[i] = c, acts[i] = a,
 *      dead[i] = (c == -1), seen[i] = (terminated[i] | truncated[i]) != 0.  Nothing else is written or counted.
 *   Otherwise:
 *   2. fresh = PW_GUIDE_AUTORESET and seen[i] != 0 -- the step that just ran reset this environment (the 0xFF flags of a refused
 *      action set seen too: exactly the set a PW_STEP_AUTORESET step resets); refused = terminated[i] == 0xFF;
 *      c_prev = cost[i].
 *   3. cut: PW_GUIDE_END_DEAD, c == -1, terminated[i] == 0, truncated[i] == 0 and not fresh: truncated[i] = 1 and
 *      episodes_ended of pw_counters advances by one (PW_PUSH_END_STUCK's rule).  A fresh state is never cut: a puzzle that is
 *      dead at its start is cut after its first step.
 *   4. shaped != NULL: F = 0 when fresh, refused, c == -2 or c_prev == -2; otherwise, with
 *      phi(x) = -(scale * (double)(x == -1 ? dead_cost[p] : x)), F = gamma * phi(c) - phi(c_prev), every operation rounded to
 *      double on its own.  shaped[i] = reward[i] + F.  reward is never written.  (dead_cost of an id outside the set counts 0.)
 *   5. counts != NULL, 0 <= p < P, not fresh, not refused; guided = c != -2 and c_prev != -2:
 *        counts[p][PW_GUIDE_GUIDED]       += 1 when guided
 *        counts[p][PW_GUIDE_OPTIMAL]      += 1 when guided, c_prev > 0 and c == c_prev - 1
 *        counts[p][PW_GUIDE_DEAD_ENTERED] += 1 when guided, c == -1 and c_prev >= 0
 *        counts[p][PW_GUIDE_UNKNOWN]      += 1 when c == -2
 *   6. cost[i] = c, acts[i] = a, dead[i] = (c == -1), seen[i] = (terminated[i] | truncated[i] after the cut) != 0.
 * n == 0 is a no-op.  Refused: a null engine; both sources or neither; acts_in without cost_in; a null puzzle_id, pos,
 * terminated, truncated, cost, acts, seen or dead; shaped without reward or dead_cost; npad not 4 / 8 / 16 / 32; n < 0; flag
 * bits other than the three; tables of another engine or without a run. */
#define PW_GUIDE_AUTORESET 1u /* the step ran with PW_STEP_AUTORESET (the same bit) */
#define PW_GUIDE_END_DEAD 2u
#define PW_GUIDE_REFRESH 4u
#define PW_GUIDE_COUNTS 4 /* GUIDED, OPTIMAL, DEAD_ENTERED, UNKNOWN */
#define PW_GUIDE_GUIDED 0
#define PW_GUIDE_OPTIMAL 1
#define PW_GUIDE_DEAD_ENTERED 2
#define PW_GUIDE_UNKNOWN 3
int pw_guide_step(PwEngine* e, PwSolveBatch* tables, int32_t* cost_in, uint8_t* acts_in, const int32_t* puzzle_id,
                  const int8_t* pos, int32_t npad, const double* reward, const uint8_t* terminated, uint8_t* truncated,
                  const uint8_t* mask, int32_t n, int32_t* cost, uint8_t* acts, uint8_t* seen, uint8_t* dead, double* shaped,
                  const int32_t* dead_cost, double gamma, double scale, int64_t* counts, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PUSHWORLD_AMD_H_ */
