/*
 * include/ifx_c_api.h -- C-ABI of libifx.so, the MI355X-native (HIP, gfx950) implementation of
 * InstanceFusion's per-frame dense surfel pipeline.
 *
 * This header is the drop-in boundary.  Every entry point names the reference
 * interface it replaces.  Citation prefixes: EF/ = elasticfusionpublic/Core/src/, IF/ = src/ of the
 * reference tree.  Plain C types only: no HIP, torch or C++ types cross the boundary.  Pointers
 * named d_* are device (HBM) pointers of the handle's GPU, every other pointer is host memory.
 *
 * Error behaviour: every function that can fail returns 0 on success and a negative IFX_E_* code
 * on failure; ifx_last_error() gives the message.  Nothing calls exit() (the reference's
 * cudaSafeCall / gpuErrChk do: EF/Cuda/convenience.cuh:64-71, IF/Core/InstanceFusionCuda.cu:11-20).
 *
 * Threading: one ifx_t = one host thread + its own HIP streams (main, frame side, loop-closure tracker); the handle is not thread-safe.
 */
#ifndef IFX_C_API_H_
#define IFX_C_API_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_NUM_INSTANCES 96   /* IF/main.cpp:31-44 (instanceNum) */
#define IFX_VOTE_FLOATS 48     /* two int16 counters per float, IF/Core/InstanceFusionCuda.cu:22-39 */

enum {
    IFX_OK = 0,
    IFX_E_INVALID = -1,   /* bad argument */
    IFX_E_HIP = -2,       /* a HIP runtime call failed */
    IFX_E_CAPACITY = -3,  /* the surfel store is full */
    IFX_E_STATE = -4      /* call not valid in the current state */
};

/* Replaces the ElasticFusion constructor arguments (EF/ElasticFusion.h:47-62, values used by
 * IF/map_interface/ElasticFusionInterface.cpp:43-45) and the Resolution/Intrinsics singletons
 * (IF/main.cpp:46-47). */
typedef struct ifx_config {
    int32_t width, height;       /* 640 x 480 */
    float fx, fy, cx, cy;        /* 528, 528, 320, 240 */
    int32_t time_delta;          /* 200 */
    float confidence;            /* 10 */
    float depth_cut;             /* 12 m */
    float max_depth_processed;   /* 20 m (EF/ElasticFusion.cpp:73) */
    float icp_weight;            /* 10 */
    int32_t pyramid;             /* 1 */
    int32_t fast_odom;           /* 0 */
    int32_t so3;                 /* 1 */
    int32_t max_surfels;         /* capacity of the surfel store (reference: 1536^2, EF/GlobalModel.cpp:22-23) */
    int32_t device;              /* HIP device ordinal */
    int32_t n_ranks, rank;       /* spatially sharded map: this handle stores shard `rank` of `n_ranks` (0 or 1: the whole map; -1: the sharded path with one rank); see ifx_owner_frame_phase */
} ifx_config;

typedef struct ifx ifx_t;

/* ---- construction (replaces `new ElasticFusion(...)`, IF/map_interface/ElasticFusionInterface.cpp:43-45) */
int ifx_create(const ifx_config* cfg, ifx_t** out);
void ifx_destroy(ifx_t* h);
const char* ifx_last_error(ifx_t* h);
/* Global (handle-free) message for failures of ifx_create itself. */
const char* ifx_global_error(void);

/* ---- frame entry.  Replaces ElasticFusion::processFrame (EF/ElasticFusion.h:75-82,
 * EF/ElasticFusion.cpp:269-720) and ElasticFusionInterface::ProcessFrame
 * (IF/map_interface/ElasticFusionInterface.h:129-130).
 * rgb: H*W*3 u8 row-major, depth: H*W u16 millimetres (0 invalid).  in_pose16: NULL to track, or a
 * row-major 4x4 camera-to-world pose to use instead of tracking.  out_pose16 (may be NULL) receives
 * currPose.  Returns 0 ok, 1 lost (option "reloc", ifx_set_option; never without it), <0 error.
 * The caller's buffers are copied during the call, which returns when the whole frame is done.
 * Option "host_entry_async" 1 (for a host whose loop is ifx_process_frame after ifx_process_frame -- a log replay without masks): the call returns when the frame's
 * POSE is known (it is read back right behind the tracker); the frame's map passes finish under the caller's next steps -- its copy of the next frame, typically
 * -- like the reference's GL work after processFrame has issued it.  Every accessor of the map, the images or the frame result waits for them, exactly as after
 * ifx_enqueue_frame_device; the housekeeping decision of the frame (compaction) is taken at the start of the next ifx_process_frame, from the same numbers; near
 * the capacity, with loop-closure detection on, with camera contexts, with an external pose and for the first frame the call synchronises fully. */
int ifx_process_frame(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, int64_t timestamp,
                      const float* in_pose16, float weight_mult, float* out_pose16);
/* The complete argument list of ElasticFusion::processFrame (EF/ElasticFusion.h:75-82).
 * inst_table: `smallInstanceTable` (96 x 5 ints, may be NULL).  Its only consumer in the reference is Ferns::findFrame
 *   (EF/ElasticFusion.cpp:468), host code that lives above this boundary (instancefusion_amd/host/ifx_ferns.hpp), so the
 *   library accepts it and does not read it -- which is why ifx_process_frame omits it.
 * bootstrap != 0: in_pose16 (required) is a GUESS, not a replacement: the model maps are placed with the current pose, then
 *   currPose = currPose * inPose is the tracker's initial estimate, and the velocity weighting compares the tracked pose with
 *   the pose before the guess (EF/ElasticFusion.cpp:330-356, :433). */
int ifx_process_frame_ex(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, int64_t timestamp, const int32_t* inst_table,
                         const float* in_pose16, float weight_mult, int bootstrap, float* out_pose16);
/* Same, with the frame already resident in HBM and no host synchronisation: the call only
 * enqueues work on the handle's stream.  Poses are appended to the device-side trajectory log.
 * With option "reloc" the call synchronises ONCE, behind the tracking gate (what it enqueues next depends on the verdict;
 * a handle with loop-closure callbacks synchronises behind its renders in the same way), announcements of the next frame
 * (ifx_hint_next_frame, ifx_hint_next_frame_device) are ignored, and it returns 1 while the map is lost. */
int ifx_enqueue_frame_device(ifx_t* h, const uint8_t* d_rgb, const uint16_t* d_depth,
                             int64_t timestamp, const float* in_pose16, float weight_mult);
/* Optional one-frame look-ahead for replayed streams (the reference's log readers know the next frame,
 * IF/utilities/RawLogReader.cpp:66-115): enqueues the part of the NEXT frame that depends only on its
 * images (copy, bilateral filter, frame pyramids, SO(3) pre-alignment against the current frame's
 * image) on a side stream, under the current frame's tracking and map passes.  Call it after
 * ifx_enqueue_frame_device for the current frame and pass the same pointers to the next
 * ifx_enqueue_frame_device; results are identical with or without it. */
int ifx_prefetch_frame_device(ifx_t* h, const uint8_t* d_rgb_next, const uint16_t* d_depth_next);
/* The same look-ahead announced BEFORE the current frame is enqueued: the next ifx_enqueue_frame_device
 * call places the announced frame's image-only work itself (behind the coarse pyramid levels of its own
 * tracker, where the GPU is least busy).  Preferred over ifx_prefetch_frame_device. */
int ifx_hint_next_frame_device(ifx_t* h, const uint8_t* d_rgb_next, const uint16_t* d_depth_next);
/* The same announcement with HOST pointers, for the reference-shaped entry: call it BEFORE ifx_process_frame of the current
 * frame, with the frame the reference's log reader would return next (IF/utilities/RawLogReader.cpp:66-115,
 * IF/main.cpp:108-307).  The buffers are borrowed for this call only (the frame is copied into pinned staging here); its
 * transfer and image-only work run on the side stream under the current frame, its tracker is parked behind the current
 * frame, and the next ifx_process_frame -- which must pass the SAME pointers; anything else and the announcement is simply
 * ignored -- finds all of that done.  Results are identical with or without it, PROVIDED the two buffers still hold at that
 * ifx_process_frame what they held here: the frame is matched by pointer identity and what was staged at the hint is what is
 * processed (a caller that refills the same buffers in between must not announce them).  Single-stream, unsharded handles. */
int ifx_hint_next_frame(ifx_t* h, const uint8_t* rgb_next, const uint16_t* depth_next);
/* ---- sharded projection for large maps.  Every rank (one process per GPU) holds the full map replica and is
 * fed the same frames and masks; the passes that stream the whole surfel store with one atomic per visible surfel (index map
 * x2, splat + id raster) only handle this rank's slice of the slots, and the ranks combine their key images between the four
 * phases of a frame by an element-wise UNSIGNED 64-bit minimum (RCCL all-reduce over xGMI; instancefusion_amd/sharded.py does
 * it through torch.distributed).  Exchange after phase 0 and after phase 1: key_index; after phase 2: key_splat, key_ids,
 * key_both; phase 3 needs none.  The replicas stay bit-identical, and identical to a single-GPU run. */
int ifx_set_shard(ifx_t* h, int rank, int nranks);
int ifx_sharded_frame_phase(ifx_t* h, int phase, const uint8_t* d_rgb, const uint16_t* d_depth);   /* pointers used by phase 0 */
int ifx_key_images(ifx_t* h, void** key_index, void** key_splat, void** key_ids, void** key_both, int64_t* n_pixels);
/* The handle's HIP streams (hipStream_t): work enqueued on the main stream between two phases (the key exchange) is
 * ordered with the phases without any host synchronisation. */
int ifx_stream_handles(ifx_t* h, void** main_stream, void** side_stream);
/* ---- spatially sharded map (BASELINE configurations 4 and 5): a handle created with ifx_config::n_ranks = G > 1 STORES only
 * the surfels it owns -- owner = Morton code of the 8 cm voxel of the position a surfel was created (or uploaded) at, mod G (ifx_owner_of) --
 * i.e. 1 / G of the map.  One process per GPU, every rank fed the same frame.  A frame is eight calls of ifx_owner_frame_phase (phase 0..7,
 * the image pointers are used by phase 0); after phase p (0..6) the caller reduces, across the ranks, the device buffers ifx_owner_exchange(p)
 * lists: ops 0 = element-wise MINIMUM of unsigned 64-bit words (key images: depth | creation number), ops 1 = SUM of 32-bit words
 * (attribute blocks with disjoint supports: the winner's rank writes a pixel, the others hold zeros); op 6 (option "own_key_rs", exchanges 0 and 2) = the MINIMUM of op 0 of which
 * only the low 32 bits of every word are wanted back -- the buffer must come back as (uint64) low word, all-ones words whole: any transport that computes op 0 and strips the
 * high words will do, the library's own runs a reduce-scatter and an all-gather of the low words (12 instead of 16 bytes per key and link direction).  The library does it itself once it holds a
 * communicator (ifx_owner_process_frame_device below); the phase / exchange pair stays for hosts with their own transport and for the emulation tests.  Poses, images and -- merged by ifx_map_seq -- the map equal the unsharded run bit for
 * bit.  Per-surfel work (projections, fusion update, clean, votes, label scan) is sharded, per-pixel work (tracking, association, the mask
 * pipeline) replicated; segmentation calls go through ifx_owner_segmentation_begin / _resume, the kNN smoothing through ifx_owner_knn_export /
 * _vote.  With the local loop-closure detection enabled (ifx_set_loop_closure; the deformation callbacks are not offered in this mode) a frame has two
 * more phases IN FRONT of phase 0 -- 300: frame side, tracker and the local ACTIVE + INACTIVE renders at the tracked pose; 301: the owners' winners of both --
 * each followed by the exchange ifx_owner_exchange(300 | 301) lists; phase 0 then runs the model-to-model tracker and the gates on the exchanged renders,
 * replicated (the same verdict on every rank, ifx_loop_closure_diag).  Both are no-ops while the detection is off or nothing can be inactive yet. */
int ifx_owner_frame_phase(ifx_t* h, int phase, const uint8_t* d_rgb, const uint16_t* d_depth);
/* ---- the same frame as ONE call, the collectives enqueued by the library itself (instancefusion_amd/csrc/ifx_comm.hip).  The reference has no
 * counterpart (one GPU, IF/main.cpp:75); BASELINE.json's north star asks for "RCCL all-reduce over xGMI ... all-to-all for cross-shard surfel
 * reprojection" with the host in C++.  The library holds a RCCL communicator (librccl.so.1 loaded with dlopen on first use: a single-GPU process
 * never maps it) and issues the exchange of every phase on the handle's main stream, between the kernels of two phases: no host round trip inside a
 * frame, six collectives per frame (u64 MIN of key images and of the association verdicts, int32 SUM of the winners' attribute blocks), 80 bytes per pixel.
 *   ifx_comm_unique_id(out128)       ncclGetUniqueId on one rank; the host hands the 128 bytes to the other ranks (MPI, a file, a socket, torch.distributed)
 *   ifx_owner_init_comm(h, id128)    ncclCommInitRank(n_ranks, id, rank) on the handle's device -- collective: every rank calls it
 *   ifx_owner_set_comm(h, comm)      adopt a ncclComm_t the host already owns (size / rank must match the handle's); NULL: back to caller-driven exchanges
 *   ifx_owner_process_frame_device   phases 0..7 + exchanges, device pointers, no synchronisation (poses: ifx_trajectory / ifx_get_pose)
 *   ifx_owner_process_frame          ElasticFusion::processFrame's shape (EF/ElasticFusion.h:75-82): host pointers, one synchronisation, currPose back
 *   ifx_owner_predict                ElasticFusion::predict outside a frame (after ifx_map_upload / ifx_set_pose)
 *   ifx_owner_process_segmentation   InstanceFusion::processInstance (IF/Core/InstanceFusion.cpp:655-1067): begin / resume with the exchanges inside; flags bit 0 also runs
 *   ifx_owner_knn_vote_colour        flannKnnVoteSurfelMap (:1070-1163): all-gather of every rank's slots (20 B each), exact 10-NN of the owned surfels
 *   ifx_owner_exchange_stats         out2 = collectives enqueued, bytes handed to them since the last reset (in all-reduce-equivalent bytes: a ring all-reduce of S bytes moves
 *                                    2 S (G - 1) / G per link direction; the reduce-scatter + all-gather pair of op 6 counts (8 + 4) / 2 bytes per key)
 * ifx_config::n_ranks = -1 creates a WORLD OF ONE on this path (creation-number ids, owner filter, every exchange point as a one-rank collective): what
 * `bench.py --sharded --gpus 1` and the single-GPU RCCL test run.
 * Creation numbers (the ids of a sharded map) are unsigned 32-bit and never renumbered: a handle reports IFX_E_CAPACITY once 2^32 - 2^20 of them have been
 * handed out (at most P / 4 per frame: > 50 000 frames at 640 x 480 in the worst case, millions in practice). */
/* ---- K streams into ONE map (BASELINE configuration 5; the reference has one stream, IF/main.cpp:75).  Semantics of a FRAME SET (one frame per camera): the K frames
 * are processed one after the other, in camera order, on the one map; a camera tracks against the prediction rendered at the end of ITS last frame.
 *   ifx_camera_count(h, K)        K camera contexts on this handle (pose block, prediction + fill-in, the last frame's intensity pyramid, id image)
 *   ifx_camera_select(h, c)       park the current camera's context, bring camera c's in (enqueue-only, between frames); a camera selected for the first time
 *                                 starts as a copy of the current one: give it its pose (ifx_set_pose) or an external pose for its first frame.  Between two
 *                                 cameras that both have a context the prediction / fill-in / id images change hands by pointer (no copies): device pointers
 *                                 obtained before the switch -- ifx_ids_after, ifx_owner_exchange lists -- are stale after it; ask again
 * On a spatially sharded map (every rank holds the K contexts and is fed all K streams):
 *   ifx_owner_set_frame_pose      the next frame takes this pose instead of tracking (the in_pose of the unsharded entry points)
 *   ifx_owner_set_tracking_rank   only this rank tracks the frames to come -- stream k on GPU k, no tracker collective; the others run the frame side,
 *                                 and the tracked pose block reaches them by a broadcast (phase 310 + ifx_owner_exchange(h, 310): op 4 | root << 8), which
 *                                 ifx_owner_process_frame_device issues itself.  -1: every rank tracks (replicated).  While a tracking rank is set the prediction
 *                                 rendered at the end of the frame has one consumer, that rank's tracker: exchange 5 lists the prediction block with op 5 | root << 8
 *                                 (int32 SUM to the root only: ncclReduce) and the 16-byte vote-mass tail with op 1 (to everybody); on the other ranks the
 *                                 prediction / fill-in images of that camera are partial and must not be read.
 * tests/test_gpu_parity.py::test_config5_two_streams_one_sharded_map: K = 2 cameras, G = 2 ranks, bit-identical to one GPU. */
int ifx_camera_count(ifx_t* h, int n_cameras);
int ifx_camera_select(ifx_t* h, int cam);
int ifx_owner_set_frame_pose(ifx_t* h, const float* pose16);
int ifx_owner_set_tracking_rank(ifx_t* h, int rank);
/* K streams, camera `cam` tracked by rank `tracking_rank` only: that rank enqueues the tracker of camera cam's NEXT frame now, on the handle's third stream, reading the
 * camera's PARKED context (prediction, fill-in, last intensity pyramid, pose block: final since the camera's last frame, untouched until its next) -- so rank k tracks camera k
 * under the other cameras' map phases instead of at the head of camera k's frame.  When that frame arrives with exactly these device pointers the parked pose block is
 * committed instead of a tracker run (same inputs and arithmetic: same pose).  Call it on every rank once camera cam's context is parked (another camera selected); the
 * other ranks return at once.  cam = -1: the number of frames whose tracker came from a run ahead so far.  (The reference has one stream and one GPU, IF/main.cpp:75.) */
int ifx_owner_track_ahead(ifx_t* h, int cam, int tracking_rank, const uint8_t* d_rgb, const uint16_t* d_depth);
int ifx_comm_unique_id(uint8_t* out128);
int ifx_owner_init_comm(ifx_t* h, const uint8_t* unique_id128);
int ifx_owner_set_comm(ifx_t* h, void* nccl_comm);
int ifx_owner_process_frame_device(ifx_t* h, const uint8_t* d_rgb, const uint16_t* d_depth, int64_t timestamp);
int ifx_owner_process_frame(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, int64_t timestamp, float* out_pose16);
int ifx_owner_predict(ifx_t* h);
int ifx_owner_process_segmentation(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks, const int32_t* class_ids, int nm, int frame, int flags);
int ifx_owner_knn_vote_colour(ifx_t* h);
int ifx_owner_exchange_stats(ifx_t* h, int64_t* out2, int reset);
/* ranks of the communicator the handle's collectives run on, as RCCL itself counts them (ncclCommCount of the communicator created by ifx_owner_init_comm or adopted
 * by ifx_owner_set_comm); 0: none yet.  What a benchmark line quotes as the number of GPUs its exchanges really crossed (no counterpart in the reference: one GPU). */
int ifx_owner_comm_ranks(ifx_t* h);
int ifx_owner_exchange(ifx_t* h, int phase, void** ptrs, int64_t* bytes, int32_t* ops, int max_n);
/* ElasticFusion::predict on the sharded map outside a frame (after ifx_map_upload / ifx_set_pose): step 0, exchange as after phase 4,
 * step 1, exchange as after phase 5, step 2. */
int ifx_owner_predict_phase(ifx_t* h, int step);
int ifx_owner_of(const float* xyz, int n, int n_ranks, int32_t* out);
/* InstanceFusion::processInstance (src/Core/InstanceFusion.cpp:655-1067) on a sharded map.  Every rank passes the same masks; what depends on a surfel's
 * votes or position is computed by its owner and merged at exchange points: _begin / _resume return 1 while one is pending -- reduce the buffers
 * ifx_owner_exchange(h, 200, ...) names (ops: 1 sum of 32-bit words, 2 minimum of signed 32-bit words, 3 maximum of signed 32-bit words), then call
 * _resume -- and 0 when the call is complete (labels of the owned surfels: ifx_labels).  flags: bit 1 superpixel refinement; the kNN smoothing (bit 0)
 * is a separate call on a sharded map (ifx_owner_knn_export / _vote).  The whetherDoSegmentation sums of a frame are complete after ifx_owner_frame_phase(h, 7, ...) (phase 6 leaves
 * the vote mass of the owned surfels in the buffer ifx_owner_exchange(h, 6, ...) names; phase 7 publishes the frame result). */
int ifx_owner_segmentation_begin(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks, const int32_t* class_ids, int nm, int frame, int flags);
int ifx_owner_segmentation_resume(ifx_t* h);
/* Option "own_lazy_ids" (ifx_set_option, sharded map only; no counterpart in the reference, whose id image -- IndexMap::renderSurfelIds, src/Core/InstanceFusion.cpp:402-466 --
 * never leaves one GPU): a frame draws and exchanges the id keys of the 10 x 10 lattice whetherDoSegmentation samples only, so exchange 4 carries
 * [splat keys | lattice keys | word] = 8 P + 8 ceil(w/10) ceil(h/10) + 8 bytes instead of 16 P + 8.  Whoever reads the whole id image completes it: a segmentation call does so
 * at an exchange point of its own in front of the others (nothing changes for the caller of _begin / _resume); ifx_image_download("ids_after"), ifx_ids_after and
 * ifx_camera_select do it in place when the library holds the communicator (ifx_owner_init_comm / _set_comm: every rank makes the same call), and return IFX_E_STATE
 * otherwise -- a caller that runs the exchanges itself calls ifx_owner_ids_begin on every rank first (1: reduce the buffer ifx_owner_exchange(h, 200, ...) names, op 0, then
 * ifx_owner_ids_resume; 0: the image is whole already). */
int ifx_owner_ids_begin(ifx_t* h);
int ifx_owner_ids_resume(ifx_t* h);
/* Option "own_track_rows" (sharded map, the library's communicator, no single tracking rank): the tracker's two reductions of an iteration (EF/Cuda/reduce.cu:257-490 ICP,
 * :494-678 photometric) run over this rank's share of the pixel blocks and the 2 x 29 exact sums are all-reduced in f64 on the handle's stream, one workgroup solves
 * (EF/Utils/RGBDOdometry.cpp:541-583).  Same poses bit for bit (the sums are exact); 38 small collectives more per frame.  Off by default: DESIGN.md section 7. */
/* InstanceFusion::flannKnnVoteSurfelMap (src/Core/InstanceFusion.cpp:1070-1163) on a sharded map: exact 10-NN over ALL surfels needs every rank's
 * positions.  ifx_owner_knn_export hands out this rank's slots as device arrays -- points[n] float4 (x, y, z, creation number; x = NaN: dead slot),
 * labels[n] int32 (bestIDInEachSurfel) --, the caller all-gathers both in rank order (16 + 4 bytes per slot, once per smoothing, i.e. every > 40
 * frames), and ifx_owner_knn_vote searches the gathered set for the surfels of this rank (own_offset = where this rank's export starts in it)
 * and recolours them.  Ties in distance go to the lower creation number: the neighbour sets of the unsharded map. */
int ifx_owner_knn_export(ifx_t* h, void** d_points, void** d_labels, int* n);
int ifx_owner_knn_vote(ifx_t* h, const void* d_all_points, const void* d_all_labels, int n_all, int own_offset);
/* creation numbers (uint32) of the live surfels in the order of ifx_map_download; returns the count */
int ifx_map_seq(ifx_t* h, uint32_t* out, int max_n);
/* ---- display / export branch of the instance layer.
 * ifx_map_bounding_boxes: InstanceFusion::computeMapBoundingBox (IF/Core/InstanceFusion.cpp:1261-1457; kernels testAllSurfelNormalVote,
 *   setGroundandInstanceCoordinate, testAllSurfelFindBBox, IF/Core/InstanceFusionCuda.cu:1555-1917): normal votes on an 18 x 36 sphere grid,
 *   ground normal = the cell with most votes, ground frame and one frame per instance (heading from the instance's own votes), boxes as
 *   min / max of the coordinates scaled by `ratio` (reference: 1e6) and truncated, in the ground frame (bbox_type 1) or the instance's
 *   (0); boxes96x6 = {minX, maxX, minY, maxY, minZ, maxZ} per instance, +-999999999 / ratio for an instance without surfels.  The optional
 *   outputs: ground normal (3), ground frame (16, row-major), instance frames (96 x 16), the 648 vote counts of the whole map.
 * ifx_instance_point_cloud: InstanceFusion::getInstancePointCloud (:1459-1590; mapCountInstanceByInstColor, getSurfelToInstanceBuffer,
 *   IF/Core/InstanceFusionCuda.cu:1920-2066): surfels per instance (counts96) and, for inst >= 0, its records {slot, x, y, z and normal in
 *   the box frame, r, g, b} (10 floats) in slot order; returns the number of records written. */
int ifx_map_bounding_boxes(ifx_t* h, int bbox_type, float ratio, float* boxes96x6, float* ground_normal3, float* gc_matrix16, float* inst_matrix96x16,
                           int32_t* ground_votes648);
int ifx_instance_point_cloud(ifx_t* h, int bbox_type, int32_t* counts96, int inst, float* out10, int max_records);
/* Diagnostics of the cached view list ("View list"): out4 = entries inside the time window, stable entries
 * outside it, scans of the store so far, frames since the last scan. */
int ifx_view_list_stats(ifx_t* h, int32_t* out4);
int ifx_sync(ifx_t* h);
/* getCurrPose(), EF/ElasticFusion.cpp:1346 / ElasticFusionInterface.h:112-115 (synchronises) */
int ifx_get_pose(ifx_t* h, float* out_pose16);
int ifx_tick(ifx_t* h);
/* Trajectory log: one pose per processed frame (ResultModel.freiburg, EF/ElasticFusion.cpp:99-136), kept on the device as a ring of
 * 65536 frames: returns the LAST min(frames processed, 65536, max_frames) poses, oldest first. */
int ifx_trajectory(ifx_t* h, float* out_poses16, int max_frames);
/* diag[8]: lastICPError, lastICPCount, lastRGBError, lastRGBCount, lastSO3Error, lastSO3Count,
 * velocity weighting, fill-in flag (EF/Utils/RGBDOdometry.h:65-70). */
int ifx_tracker_diag(ifx_t* h, float* diag8);
/* Pyramid levels that the persistent Gauss-Newton kernel (option gn_persist) could not finish because a meeting of its workgroups did not happen (the grid was
 * not co-resident: other work held the GPU) and that one workgroup re-ran alone inside the same frame -- same sums, same solve, same pose, only slower.  A count since
 * ifx_create, >= 0; negative: error.  Replaces nothing of the reference (its tracker reads every reduction back, EF/Utils/RGBDOdometry.cpp:461-583): a diagnostic
 * of this implementation's schedule.  Waits for the frames in flight. */
int ifx_tracker_fallbacks(ifx_t* h);
/* Run-time guard of the tracker's exact sums: the number of reductions, since ifx_create, whose diagonal totals left the range in which every addition of the normal-equation
 * sums is exact (2^53 units of the entry's grid; tested at half of it).  While it is 0 the sums -- and with them every pose -- are independent of the order in which blocks and
 * atomics arrive and equal to the CPU oracle's; a non-zero count names frames (saturated edges at near range, magnitudes ~2^7 above what real RGB-D data produces) whose poses
 * may differ from run to run in the last bit.  >= 0; negative: error.  Replaces nothing of the reference (its reductions are f32 trees whose shape depends on the GPU,
 * EF/Utils/GPUConfig.h:53-137: no order-independence to guard).  Waits for the frames in flight. */
int ifx_tracker_range_exceeded(ifx_t* h);
/* photometric blocks of fused tracker iterations (option "rgb_fuse") that stopped waiting at their bounded meeting since ifx_create (0 in a healthy run; the poses do not depend on it) */
int ifx_tracker_meet_giveups(ifx_t* h);
/* shares of such blocks that the last arriver of the meeting stepped in their place (option "rgb_own": a block steps the records it wrote, and one that leaves hands them
 * over); equal to ifx_tracker_meet_giveups while every fused launch runs that form, 0 in a healthy run */
int ifx_tracker_meet_adopted(ifx_t* h);

/* ---- local loop-closure DETECTION (the closeLoops / countThresh / errThresh / covThresh constructor arguments, EF/ElasticFusion.h:48-51;
 * EF/ElasticFusion.cpp:453-566 with no fern match).  When enabled every tracked frame also runs predict() at the new pose, the INACTIVE
 * prediction (surfels not seen for time_delta frames), the model-to-model tracker (RGBDOdometry modelToModel: active render against
 * inactive render, ICP weight 10, no SO(3)) and the gates covariance diagonal <= cov_thresh, lastICPCount > count_thresh, lastICPError <
 * err_thresh.  The reference then deforms the map (deformation graph) and adopts the estimated pose: the GPU half of that is provided by
 * the hooks below (ifx_set_loop_closure_callback ... ifx_adopt_estimated_pose), the graph optimiser is host code above this boundary
 * (instancefusion_amd/host/ifx_deformation.hpp).  Without a callback an accepted candidate is counted and reported and the frame
 * continues with the tracked pose; a run whose candidate count stays 0 is what the reference computes with closeLoops = true.
 * out24: 0 model-to-model ran (0: nothing inactive in view), 1 pixels of the inactive render, 2 lastICPError, 3 lastICPCount, 4 covOk,
 * 5 accepted, 6..21 estimated pose (row-major 4x4), 22 largest diagonal covariance entry, 23 candidates accepted so far. */
int ifx_set_loop_closure(ifx_t* h, int enable, int count_thresh, float err_thresh, float cov_thresh);
int ifx_loop_closure_diag(ifx_t* h, float* out24);
/* ---- hooks for the deformation that follows an accepted candidate (EF/ElasticFusion.cpp:566-613).  The graph OPTIMISATION is host code
 * of the reference (Deformation / DeformationGraph: Eigen + cholmod) and stays with the caller; the library provides what touched the GPU:
 * ifx_set_loop_closure_callback: cb runs inside ifx_process_frame / ifx_enqueue_frame_device right after the gates of a frame whose candidate
 *   was accepted (the frame waits for the verdict: one host synchronisation per frame while a callback is set).  From the callback:
 * ifx_sample_graph_model: Deformation::sampleGraphModel (EF/Deformation.cpp:224-337, sample.geom): x, y, z, init time of every 5000th surfel
 *   of the map order (the map state is the one the reference samples at the end of the previous frame); returns the number written.
 * ifx_loop_closure_constraints: the samples of :568-598 -- ACTIVE vertex render and INACTIVE time render on a (w/20) x (h/20) grid; per valid
 *   sample worldRawPoint = currPose * v (src3), worldModelPoint = estPose * v (dst3) and the surfel time (times); returns the count.
 * ifx_set_deformation: the `graph` argument of GlobalModel::clean (EF/GlobalModel.cpp:700-760): n_nodes x 16 floats (position 3, rotation 9
 *   column-major, translation 3, time), sorted by time, 4 <= n_nodes < 1024.  The NEXT clean (of this frame when called from the callback)
 *   applies it to every surviving surfel not created in that frame (copy_unstable.vert:178-374) and, for a local loop closure
 *   (is_fern = 0), refreshes the time stamp of moved stable surfels in front of the re-rendered INACTIVE depth (IndexMap::synthesizeDepth).
 * ifx_adopt_estimated_pose: currPose = estPose (:606). */
typedef int (*ifx_loop_closure_cb)(ifx_t* h, const float* lc24, void* user);
int ifx_set_loop_closure_callback(ifx_t* h, ifx_loop_closure_cb cb, void* user);
int ifx_sample_graph_model(ifx_t* h, float* out_xyzt, int max_n);
int ifx_loop_closure_constraints(ifx_t* h, float* src3, float* dst3, int32_t* times, int max_n);
int ifx_set_deformation(ifx_t* h, const float* graph16, int n_nodes, int is_fern);
int ifx_adopt_estimated_pose(ifx_t* h);

/* ---- the GPU contacts of the fern data base (EF/Ferns.cpp; codes, similarity search and keyframe store are host code in the reference and here:
 * instancefusion_amd/host/ifx_ferns.hpp is that class over the entry points below).
 * ifx_fern_frame: the four Resize passes of Ferns::addFrame / findFrame (:95-98, :192-195): fill-in image / vertex / normal and the instance render of the
 *   last predict(), resampled to (w/8) x (h/8) and read back (rgb: 3 bytes, maps: float4 per sample); returns the number of samples.
 * ifx_track_maps: the texture-initialised tracker as a stage -- initICPModel / initRGBModel(model maps, given in the frame of pose16) + initICP(vertices,
 *   normals) / initRGB(current maps) + getIncrementalTransformation starting at pose16 (EF/Ferns.cpp:558-592, EF/ElasticFusion.cpp:528-545).  Host
 *   float4 maps of the handle's resolution (RGBA8 images or NULL); uses the handle's configuration (icp_weight, pyramid, fast_odom; no SO(3)): for
 *   ferns create a handle with width/8, height/8, intrinsics/8, icp_weight 100, pyramid 0.  pose16 in: model pose = initial estimate; out: estimate.
 *   diag8: lastICPError, lastICPCount, lastRGBError, lastRGBCount, 0...
 * ifx_set_fern_callback: where the reference looks its fern data base up and deforms globally (EF/ElasticFusion.cpp:457-514): every frame after the
 *   first, with loop closure enabled, right after predict() at the tracked pose and before the local detection.  Inside the callback ifx_fern_frame
 *   delivers that predict() (what findFrame resamples), ifx_set_deformation(is_fern = 1) hands the optimised graph to this frame's clean and
 *   ifx_adopt_pose sets currPose = recoveryPose (:482, :504).  Return 1 when a graph was produced (rawGraph.size() > 0: the local detection of this
 *   frame is skipped, :516), 0 otherwise, < 0 to fail the frame.  A handle with this callback synchronises once per frame, as the reference does.
 *   Outside the callback ifx_fern_frame delivers the end-of-frame predict() (what Ferns::addFrame stores, :713-716). */
typedef int (*ifx_fern_cb)(ifx_t* h, void* user);
int ifx_set_fern_callback(ifx_t* h, ifx_fern_cb cb, void* user);
int ifx_adopt_pose(ifx_t* h, const float* pose16);
int ifx_fern_frame(ifx_t* h, uint8_t* img_rgb, float* verts4, float* norms4, uint8_t* inst_rgb);
/* the end-of-frame read-back (Ferns::addFrame) without a host stall: _async enqueues it behind the frame just processed, _fetch waits for it and hands
 * the four images over -- typically at the start of the next frame's fern callback, where the host has to wait for the stream anyway */
int ifx_fern_frame_async(ifx_t* h);
int ifx_fern_frame_fetch(ifx_t* h, uint8_t* img_rgb, float* verts4, float* norms4, uint8_t* inst_rgb);
int ifx_track_maps(ifx_t* h, const float* model_v4, const float* model_n4, const uint8_t* model_rgba, const float* cur_v4, const float* cur_n4,
                   const uint8_t* cur_rgba, float* pose16, float* diag8);

/* ---- map access (replaces getMapSurfelsGpu / getMapSurfelCount / id textures,
 * IF/map_interface/ElasticFusionInterface.h:55-120).  The store is struct-of-arrays; slots whose
 * surfel was deleted stay in place as tombstones until ifx_compact (DESIGN.md "Tombstones"). */
typedef struct ifx_soa_view {
    int32_t count;          /* slots in use (including tombstones) */
    int32_t capacity;
    float* d_pos_conf;      /* [capacity] float4: x,y,z, confidence          (vPosition)   */
    float* d_norm_rad;      /* [capacity] float4: nx,ny,nz, radius           (vNormRad)    */
    float* d_color;         /* [capacity] float2: packed rgb, packed inst.   (vColor.xy)   */
    float* d_times;         /* [capacity] float2: init time, last time       (vColor.zw)   */
    float* d_img_corr;      /* [capacity] float4                             (vImgCorr)    */
    float* d_votes;         /* [capacity][48]: vInstInfoA..L, one 192-byte record per slot */
} ifx_soa_view;
/* The pointers are MUTABLE, like the reference's getMapSurfelsGpu (its instance kernels write votes and colours through it), and a view is valid UNTIL THE NEXT FRAME
 * CALL on the handle: the frame path keeps a gathered copy of position / normal / times per slot ("hot records") that it rebuilds after every
 * ifx_map_view, so writes made between this call and the next frame are seen; writes through a pointer kept PAST a frame call are not (the list passes would read the
 * stale copy while the scans read the arrays) -- call ifx_map_view again before such writes.  ifx_set_option(h, "hot_verify", 1) makes every frame compare the copy with
 * the arrays first (one streaming pass, debug only); ifx_hot_records_stale returns how many slots it found differing (and repaired) since ifx_create: 0 for a caller
 * that keeps the rule.
 * The arrays are AS OF THE REFERENCE'S CLEAN PASS of the last frame: the call first applies the age rule to every slot the cached view list leaves out (the forced scan
 * every whole-store reader makes, ifx_map.hip "View list"), so a slot whose times.y is above the tombstone marker is a surfel the reference's map holds, and no other. */
int ifx_map_view(ifx_t* h, ifx_soa_view* out);
int ifx_hot_records_stale(ifx_t* h);
int ifx_map_count(ifx_t* h);      /* live surfels (synchronises) */
int ifx_map_slots(ifx_t* h);      /* slots incl. tombstones (synchronises) */
/* Host copies of the live surfels in map order.  pc,nr,ic: float4 per surfel; col,tm: float2;
 * votes: 48 floats per surfel.  Any pointer may be NULL.  Returns the number of surfels written. */
int ifx_map_download(ifx_t* h, int max_n, float* pc, float* nr, float* col, float* tm, float* ic,
                     float* votes);
int ifx_map_upload(ifx_t* h, int n, const float* pc, const float* nr, const float* col,
                   const float* tm, const float* ic, const float* votes);
int ifx_set_pose(ifx_t* h, const float* pose16, int tick);
int ifx_compact(ifx_t* h);        /* order-preserving removal of tombstones */
/* Runtime options (name, value):
 *   "pyramid" / "fast_odom" / "so3" (0|1), "icp_weight_x1000" -- ElasticFusion::setPyramid / setFastOdom / setSo3 / setIcpWeight (EF/ElasticFusion.h:153-176), from the
 *                           next frame on; refused while a frame is announced ahead
 *   "reference_passes" 1  -- also run the BEFORE / INSTANCECOMPARE id renders of EF/ElasticFusion.cpp:679-680 (nobody on this path consumes them)
 *   "compact_every_frame" 1 -- remove tombstones after every clean (tests); "compact_divisor" d -- housekeeping compaction when tombstones > slots / d (default 8)
 *   "two_streams" 0       -- everything on one stream; "track_ahead" 0 -- do not enqueue the announced frame's tracker behind the current frame; "slic_ahead" 0 -- no superpixels ahead of a call
 *   "stage_timing" / "kernel_timing" 1 -- HIP-event records for ifx_stage_ms / ifx_kernel_ms (cost frame rate: off by default)
 *   "icp_blocks" n        -- cap on the blocks of a tracker reduction launch (0 = by image size)
 *   "raster_tiles" -1|0|1 -- tiled rasteriser (key tiles in LDS): by image size (on from 1 Mpixel) | off | on; results are identical either way
 *   "pace" 0              -- ifx_enqueue_frame_device normally waits for the PREVIOUS frame's result before it enqueues (the tracker announced ahead keeps the
 *                           device busy meanwhile); 0 = enqueue without looking back (a host that runs frames ahead measured 25 % slower)
 *   "gn_persist" mask     -- bit i: the Gauss-Newton iterations of pyramid level i in one persistent launch with grid barriers, while that level's grid has at
 *                           most "gn_persist_blocks" blocks (default 128).  Default 0 below 1280x960 (the two-launch form with the solve in the next launch's
 *                           prologue is within 0.7 % there and needs no co-resident grid), 4 = the coarsest level from 1280x960 on (+5 %).  A meeting of its
 *                           blocks that does not happen is re-run by one workgroup inside the frame (ifx_tracker_fallbacks counts them): slower, never wrong.
 *   "rgb_cand" 0          -- the photometric term of the frame-to-model tracker over every pixel (the dense passes) instead of over the frame slot's candidate
 *                           list; same bits.  A run with a persistent level ("gn_persist") or row-sharded reductions is dense whatever the option says
 *   "rgb_fuse" mask       -- a bit per pyramid level: in list runs ("rgb_cand") the photometric step of a prologue-chain iteration runs inside the iteration's
 *                           residual launch (its photometric blocks meet, bounded, and step the records by claimed chunks); same bits.  0: two launches per
 *                           iteration.  "rgb_fuse_poll" 0 (test switch) -- no block waits at that meeting: the last arriver steps every chunk alone
 *                           (ifx_tracker_meet_giveups counts the blocks that left)
 *   "rgb_own" mask        -- a bit per pyramid level: in a fused iteration ("rgb_fuse") every photometric block steps the records it wrote itself, the first of
 *                           each thread from registers, instead of claiming chunks; a block that stops waiting at the meeting hands its share to the last
 *                           arriver (ifx_tracker_meet_adopted); same bits.  0: chunk claims.  Launches with more than 64 photometric blocks ("rgb_blocks")
 *                           run the chunk form
 *   "gn_prologue" 0       -- the 6x6 solve of an iteration by the last block of its second launch (round 3's form) instead of by every block of the next
 *                           iteration's first launch; "gn_prologue_blocks" n -- the prologue form only for launches of at most n blocks (default 2048)
 *   "fold_result" 0       -- the frame result by a launch of its own instead of the last block of the prediction's resolve
 *   "lazy_ids" 0          -- render the whole id image every frame (default: the lattice whetherDoSegmentation samples; the rest on demand)
 *   "id_rule" 0|1         -- the id renders of an unsharded map (the frame's ids_after, dense or lattice, and its on-demand completion; the BEFORE / INSTANCECOMPARE
 *                           renders of "reference_passes"; both modes of ifx_render_ids): 0 (default) a ray through each pixel centre against the disc, f32
 *                           depth keys; 1 the reference's rule -- surfel_ids.geom's screen-space quad, texcoord interpolated affinely, dot > 1 discarded,
 *                           24-bit depth with GL_LESS (ties: the lower slot) -- the reference's id images up to GL's sub-pixel latitude (DESIGN.md section 9-3
 *                           has its cost).  Refused (IFX_E_STATE) on a sharded handle and while a frame is in flight or announced ahead; a change re-renders
 *                           the current id image at once.  Not the INACTIVE splat of the loop-closure detection, which is a splat render.
 *   "seg_device" 0, "seg_aside" 0, "ff_rounds" n -- the earlier forms of the segmentation call's schedule (host-driven / on the main stream) and the length
 *                           of the flood fill's fixed relaxation schedule (default 4); identical results
 *   "compare_map" 1|2     -- how a segmentation call matches a mask to a map instance (the reference's compareMapType, IF/Core/InstanceFusion.h:227): 1 (default)
 *                           box IoU, computeCompareMap (IF/Core/InstanceFusion.cpp:595-651); 2 mask IoU over 3 x 3-dilated pixel sets, the reference's "PLAN B"
 *                           (maskCompareMapKernel, IF/Core/InstanceFusionCuda.cu:826-881; the decision, IF/Core/InstanceFusion.cpp:805-870) -- see
 *                           ifx_mask_compare_map for the rule.  At 2 every entry that runs the call's body on an unsharded handle uses it, under both
 *                           schedules ("seg_device") with identical results, and the recompute after an eviction uses it too (the reference falls back to the
 *                           box rule there: DESIGN.md section 1).  Any other value: IFX_E_INVALID.  2 on a sharded handle, and ifx_set_shard(n > 1) while
 *                           the option is 2: IFX_E_STATE (dilated presence is not additive over ranks).  Cost at 640x480 / 5 M surfels / the bench's 8 masks:
 *                           +46 .. +51 us on a call of 0.40 ms (0.63 with superpixels) -- the presence pass 59-61 us in the place of the instance-box pass's 47-49,
 *                           the count kernel 36-37 us (99-100 at 100 masks), the decision 7.7 for 6.4-7.2; the reference's remark for its own version is
 *                           10 - 330 ms per call.  With the option at 1 the call is the parent's within the spread between runs (profiles/r23_compare_map_iou.txt)
 *   "clean_raster" 0, "hot_records" 0 -- round 5's map-pass forms off: the clean pass and the prediction's raster as ONE walk of the view list; the
 *                           gathered 64-byte copy of the hot fields.  Identical results
 *   "host_entry_async" 1  -- ifx_process_frame returns when the frame's POSE is known (see there)
 *   "seg_snapshots" n     -- outstanding tickets of ifx_segmentation_snapshot allowed at a time, 1..8 (default 4)
 *   "own_first_live" 0    -- test switch: the sharded map's "surfel 0" fixed at creation number 0 (round 4's behaviour: results then differ from the
 *                           reference's in the cases test_owner_sharded_map_emulated holds)
 * An unknown name is refused (IFX_E_INVALID); ifx_create reports each entry of IFX_OPTS that is refused on stderr and goes on. */
int ifx_set_option(ifx_t* h, const char* name, int value);
/* Options "reloc" and "frame_to_frame_rgb" (0 | 1): the `reloc` and `frameToFrameRGB` arguments of the ElasticFusion constructor
 * (EF/ElasticFusion.h:47-62), which replace "kept for the getter only" and the constructor's throw of host/ifx_host.hpp.
 * IFX_E_STATE on a sharded handle, with camera contexts, and while a frame is in flight or announced.
 *   reloc: every tracked or bootstrapped frame is judged behind its tracker (ifx_reloc_gate's rule; a frame with an external pose
 *   is not, EF/ElasticFusion.cpp:334, :428-431).  The pose is adopted whatever the verdict (:425-426).  A frame that is not ok, or
 *   any frame while lost, runs no index map, fusion, clean or id render (:620): the id image stays the last fused frame's.  While
 *   lost the local loop-closure detection is skipped (:516), the fern callback sees the raw frame (ifx_fern_frame: passthrough 3),
 *   ifx_adopt_pose from it also sets lastFrameRecovery (:480-484), the tick stands still (:713-717) and the frame entries return 1;
 *   with lastFrameRecovery both predict() calls take the time window (0, tick) (:733-754).  The trajectory takes a pose every frame.
 *   frame_to_frame_rgb: the photometric term's model image is the fill-in image whatever the dense test says (:346), and that image is
 *   the previous raw frame (passthrough 2, :759).
 * ifx_reloc_state: out12 = {ok, lost, lastFrameRecovery, trackingCount, lastICPError, the six covariance diagonals (as float),
 * 1 if the last frame ran its map passes}; waits for the last frame. */
int ifx_reloc_state(ifx_t* h, float* out12);

/* R32I surfel-id image after fusion (getSurfelIdsAfterFusionGpu, ElasticFusionInterface.h:90-102):
 * linear H*W int32 device buffer, 0 = empty. */
const int32_t* ifx_ids_after(ifx_t* h);
/* Host copy of an internal image (synchronises).  Names: "ids_after", "ids_tmp", "index",
 * "index_vc", "index_ct", "index_nr", "pred_vertex", "pred_normal", "pred_image", "pred_inst",
 * "pred_time", "fill_vertex", "fill_normal", "fill_image", "depth_filtered", "depth_metric",
 * "depth_metric_filtered", and with loop-closure detection on "old_vertex", "old_normal", "old_image", "old_time" (the
 * INACTIVE prediction, IndexMap::oldVertexTex() etc.) and "act_vertex", "act_normal", "act_image" (the predict() of
 * EF/ElasticFusion.cpp:453).  Returns bytes written or <0. */
int ifx_image_download(ifx_t* h, const char* name, void* out, int64_t max_bytes);

/* ---- map stage API (unit-parity surface; each replaces one GL pass of the reference) */
int ifx_predict_indices(ifx_t* h, const float* pose16, int time);                /* EF/IndexMap.cpp:221-279 */
int ifx_combined_predict(ifx_t* h, const float* pose16, int time, int max_time); /* EF/IndexMap.cpp:468-574 */
/* The same pass with the fill-in stage's `passthrough` uniform (fill_vertex / fill_normal / fill_rgb.frag,
 * EF/Shaders/FillIn.cpp:65-195, called with it at EF/ElasticFusion.cpp:757-759).  passthrough_mask bit 0: fill_vertex and
 * fill_normal take the frame (vertex from the filtered depth, normal from its +x / +y neighbours) at every pixel; bit 1:
 * fill_image takes the frame's colour, alpha 255, at every pixel.  An output whose bit is clear keeps the passthrough = 0
 * rule; pred_* are never touched.  The reference passes 3 while lost and 2 with frameToFrameRGB.  Mask 0 is
 * ifx_combined_predict; a mask outside 0..3 is IFX_E_INVALID. */
int ifx_combined_predict_ex(ifx_t* h, const float* pose16, int time, int max_time, int passthrough_mask);
/* The tracking gate of the relocalisation mode (reloc = true), EF/ElasticFusion.cpp:371-423 with RGBDOdometry::getCovariance
 * (EF/Utils/RGBDOdometry.cpp:605-608), as a stage on the device.  lastA36: the tracker's last normal matrix, row-major f64;
 * icp_error: its lastICPError; state3_inout: {lost, lastFrameRecovery, trackingCount}, updated in place.
 *   ok = icp_error < 1e-4f (a NaN is not ok);
 *   not lost: a diagonal of lastA^-1 > 1e-04 (f64) clears ok; not ok counts up and the count passing 10 sets lost, ok clears the count;
 *   lost with lastFrameRecovery: the same covariance test; ok clears lost and the count; lastFrameRecovery is cleared either way;
 *   lost without it: the state is untouched.
 * ok_out (may be null): the verdict; cov_diag6 (may be null): the six diagonals of lastA^-1, reported in every branch. */
int ifx_reloc_gate(ifx_t* h, const double* lastA36, float icp_error, int32_t* state3_inout, int32_t* ok_out, double* cov_diag6);
int ifx_fuse(ifx_t* h, const float* pose16, int time, float weighting);          /* EF/GlobalModel.cpp:459-698 */
int ifx_clean(ifx_t* h, const float* pose16, int time);                          /* EF/GlobalModel.cpp:700-925 */
int ifx_render_ids(ifx_t* h, const float* pose16, int mode);                     /* EF/IndexMap.cpp:315-465; result in "ids_tmp" */
int ifx_set_frame(ifx_t* h, const uint8_t* rgb, const uint16_t* depth);          /* upload + preprocess only */

/* ---- tracker stage API (replaces the blocking host launchers of EF/Cuda/cudafuncs.cuh:64-183).
 * All pointers are device pointers; planar maps are [3][h][w]; results go to device memory. */
int ifx_icp_step(ifx_t* h, const float* Rcurr9, const float* tcurr3, const float* d_vmap_curr,
                 const float* d_nmap_curr, const float* Rprev_inv9, const float* tprev3, float fx,
                 float fy, float cx, float cy, const float* d_vmap_g_prev, const float* d_nmap_g_prev,
                 float dist_thres, float angle_thres, int w, int hgt, float* out29_host);
int ifx_rgb_residual(ifx_t* h, float min_scale, const int16_t* d_didx, const int16_t* d_didy,
                     const float* d_last_depth, const float* d_next_depth, const uint8_t* d_last_img,
                     const uint8_t* d_next_img, void* d_corres8, float max_depth_delta,
                     const float* kt3, const float* krkinv9, int w, int hgt, int* count_host,
                     int* sigma_host);
int ifx_rgb_step(ifx_t* h, const void* d_corres8, float sigma, const float* d_cloud3, float fx,
                 float fy, const int16_t* d_didx, const int16_t* d_didy, float sobel_scale, int w,
                 int hgt, float* out29_host);
int ifx_so3_step(ifx_t* h, const uint8_t* d_last_img, const uint8_t* d_next_img,
                 const float* image_basis9, const float* kinv9, const float* krlr9, int w, int hgt,
                 float* out11_host);
/* The pyramid builders as ONE stage call: createVMap / createNMap / pyrDown / pyrDownGaussF / pyrDownUcharGauss / resizeVMap / resizeNMap / tranformMaps /
 * verticesToDepth / imageBGRToIntensity / computeDerivativeImages / projectToPointCloud (EF/Cuda/cudafuncs.cuh:64-183), chained as RGBDOdometry::initICP + initRGB
 * (the frame side: EF/Utils/RGBDOdometry.cpp:118-142, 243-247, 287-293) and initICPModel + initRGBModel (the model side: :169-206, 237-241) chain them.
 * In (device): the bilateral-filtered depth (u16 millimetres, DEPTH_FILTERED) and the RGB8 frame -- both or neither; the model prediction as float4 vertex / normal
 * maps in the camera frame of `model_pose16` (host, row-major camera-to-world) and its RGBA8 image -- all three or none.
 * Out (device, caller-allocated, DENSE: pitch = the level's width; the reference's DeviceArray2D are pitched, its kernels address them by row all the same): level l
 * is (width >> l) x (height >> l); planar maps are [3][h_l][w_l].  A NULL entry is skipped.  The handle's own pyramids are overwritten (it is a stage call, like
 * ifx_track_pair); the depth cut-off of createVMap is the handle's max_depth_processed (EF/ElasticFusion.cpp:73), that of verticesToDepth 6 m as in the reference.
 * Error behaviour: IFX_E_INVALID for a half-given input group, IFX_E_STATE for a point cloud at a level the handle's configuration never iterates on. */
typedef struct ifx_pyramids {
    /* frame side */
    uint16_t* depth[3];        /* depth_tmp: level 0 = the input, then pyrDown (5x5 Gaussian with the 3-sigma depth gate)          [h_l][w_l]    */
    float* vmap_curr[3];       /* createVMap                                                                                       [3][h_l][w_l] */
    float* nmap_curr[3];       /* createNMap                                                                                       [3][h_l][w_l] */
    uint8_t* next_img[3];      /* imageBGRToIntensity, pyrDownUcharGauss                                                           [h_l][w_l]    */
    int16_t* didx[3];          /* computeDerivativeImages (Sobel x)                                                                [h_l][w_l]    */
    int16_t* didy[3];          /* computeDerivativeImages (Sobel y)                                                                [h_l][w_l]    */
    /* model side */
    float* vmap_g_prev[3];     /* copyMaps, resizeVMap, tranformMaps: vertices in the GLOBAL frame                                 [3][h_l][w_l] */
    float* nmap_g_prev[3];     /* copyMaps, resizeNMap, tranformMaps                                                               [3][h_l][w_l] */
    float* last_depth[3];      /* verticesToDepth, pyrDownGaussF                                                                   [h_l][w_l]    */
    uint8_t* last_img[3];      /* intensity of the predicted image, pyrDownUcharGauss                                              [h_l][w_l]    */
    float* cloud[3];           /* projectToPointCloud                                                                              [h_l][w_l][3] */
} ifx_pyramids;
int ifx_build_pyramids(ifx_t* h, const uint16_t* d_depth_filtered, const uint8_t* d_rgb, const float* d_model_v4, const float* d_model_n4, const uint8_t* d_model_rgba,
                       const float* model_pose16, ifx_pyramids* out);
/* Whole tracker on explicit inputs (RGBDOdometry::initICPModel/initRGBModel/initICP/initRGB +
 * getIncrementalTransformation, EF/Utils/RGBDOdometry.cpp:118-603).  Host inputs. */
int ifx_track_pair(ifx_t* h, const float* model_v4, const float* model_n4, const uint8_t* model_rgba,
                   const uint8_t* prev_rgb, const uint16_t* depth_filtered, const uint8_t* rgb,
                   float* pose16_inout, float* diag8);
/* Host copy of a tracker pyramid buffer; names as in the reference's members
 * (EF/Utils/RGBDOdometry.h:80-121): "vmap_curr","nmap_curr","vmap_prev","nmap_prev","last_depth",
 * "last_img","next_img","lastnext_img","didx","didy","cloud","corres","depth_tmp"; and of the bound frame slot "cand_n" (4 bytes: the number of candidate
 * pixels of the photometric term at this level) and "cand" (w * h entries of 8 bytes {uint32 pixel, int16 gx, int16 gy}, the first cand_n valid, in no
 * particular order; with option "rgb_cand" the frame-to-model tracker's "corres" holds record t for entry t). */
int ifx_tracker_buffer_download(ifx_t* h, const char* name, int level, void* out, int64_t max_bytes);

/* ---- instance layer (replaces InstanceFusion::whetherDoSegmentation / ProcessSegmentation /
 * processInstance, IF/Core/InstanceFusion.h:72-107, IF/Core/InstanceFusion.cpp:192-270,655-1067) */
int ifx_should_segment(ifx_t* h, int frame);
/* masks: n x H x W u8 (0/255), sorted by area descending (the contract of the Mask-RCNN bridge,
 * build/mask_ori.py:117); class_ids: n COCO indices.  flags bit0: kNN smoothing of the instance colours
 * (isflann: flannKnnVoteSurfelMap, IF/Core/InstanceFusion.cpp:1070-1163), bit1: superpixel refinement (needs rgb and depth of the frame: host pointers, as
 * InstanceFusion::ProcessSegmentation takes them -- or BOTH NULL = the frame most recently processed, whose raw images are still resident in their frame slot:
 * no staging copy, no upload).
 * Refusals (this entry and ifx_process_segmentation_deferred alike): IFX_E_INVALID with ifx_last_error "<entry>: n must be 0 .. 256" for n < 0 or n > 256, and
 * "<entry>: null masks or class ids" for a NULL pointer with n > 0. */
int ifx_process_segmentation(ifx_t* h, const uint8_t* rgb, const uint16_t* depth,
                             const uint8_t* masks, const int32_t* class_ids, int n, int frame,
                             int flags);
/* The same call on a detector's raw output already in device memory of the handle's GPU (a PyTorch detector on the same device: no download, no host sort).
 * d_masks: n x H x W elements, contiguous, in ANY order ([N,1,H,W] is the same layout).  mask_format IFX_MASK_U8: a pixel is inside iff its byte is non-zero
 * (bool / uint8 masks, the host entry's 0/255); IFX_MASK_F32: inside iff its value is > threshold (mask probabilities as paste_mask_in_image thresholds them;
 * NaN is outside); threshold is ignored for U8.  d_class_ids: n int32 (device), each follows its mask.  The call applies the bridge's two steps on the device
 * (build/mask_ori.py:87-124): binarise to 0/255, then a STABLE sort by inside-pixel count, descending (ties keep their input order).  flags: as above; the frame
 * is always the resident one (rgb = depth = NULL above; the superpixel look-ahead serves it the same way).  stream: the HIP stream the producer wrote on
 * (NULL = the null stream): the call orders itself behind it with an event wait and does not synchronise the host on it.  Like the host entry, the call returns
 * after its work has finished: the buffers may then be reused or freed.
 * Result: bit for bit that of ifx_process_segmentation(h, NULL, NULL, bridge(masks), bridge(class_ids), n, frame, flags).
 * Refusals (nothing enqueued, the handle stays usable): IFX_E_INVALID for n < 0, n > 256, an unknown format or NULL pointers with n > 0; IFX_E_STATE on a
 * sharded handle (n_ranks > 1 or -1, ifx_set_shard), whose masks go through ifx_owner_process_segmentation. */
enum { IFX_MASK_U8 = 0, IFX_MASK_F32 = 1 };
int ifx_process_segmentation_device(ifx_t* h, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids, int n, int frame, int flags,
                                    void* stream);
/* ifx_ingest_masks: the ingestion of ifx_process_segmentation_device alone, as a stage (the twin of ifx_paste_roi_masks below): same arguments, checks and
 * launches; downloads to HOST pointers that may be NULL: the 0/255 masks in the bridge's order, the same after the overlap clean, the order, the class ids. */
int ifx_ingest_masks(ifx_t* h, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids, int n, void* stream, uint8_t* out_ori,
                     uint8_t* out_clean, int32_t* out_order, int32_t* out_class_ids);
/* ---- deferred segmentation: a detector slower than the frame loop (no counterpart in the reference, whose detector thread is switched off at IF/main.cpp:83, so that
 * its masks always belong to the frame processed last).  ifx_process_segmentation[_device] reads the CURRENT id image, the CURRENT pose and the RESIDENT frame; a real
 * Mask R-CNN needs tens of milliseconds per image, i.e. dozens of frames.  The pair below makes a late call well-defined without stalling the frame loop; nobody who
 * does not call it sees any difference.
 * ifx_segmentation_snapshot: pins what a call reads of the frame processed last -- its whole id image (whatever "id_rule" / "lazy_ids" drew), held as CREATION NUMBERS
 *   (ifx_map_seq: ascending in map order, carried by compaction, never reused), its pose, and with flags bit 1 its raw rgb / depth for the superpixel refinement (copied
 *   device to device; 8 + 5 bytes per pixel and snapshot).  Enqueue-only on the handle's main stream: no host synchronisation.  Returns a ticket >= 0.  Buffers for the
 *   outstanding tickets are allocated on first use; option "seg_snapshots" (1..8, default 4) is the limit; one more returns IFX_E_CAPACITY.
 * ifx_process_segmentation_deferred[_device]: at any later time, the ordinary call's pipeline, unchanged, on the map as it is NOW (votes, positions, instance table, label
 *   state), with three inputs replaced.  (1) The id image is the snapshot's, re-addressed in today's slots: a pixel keeps its surfel if that surfel is still in the store;
 *   it reads 0 ("no surfel") if the surfel was compacted away, is a tombstone, or is today's first live slot (the reference's "surfel 0" is never voted for).  Surfels
 *   created since are in no pixel of that image and get no votes.  (2) The camera centre of the model-depth step (getProjectDepthMap, IF/Core/InstanceFusion.cpp:977-996)
 *   is the snapshot's pose.  (3) The superpixels (flags bit 1) are cut from the snapshot's frame.  masks / class_ids / n / frame / flags and d_masks ... stream: as for
 *   ifx_process_segmentation / _device, with the same argument checks.  With no frame in between the result is bit for bit the ordinary call's.  The device schedule is
 *   used whatever "seg_device" says (identical results).  A successful call releases its ticket; n == 0 or an empty map releases it and is a no-op.
 * ifx_segmentation_snapshot_release: gives a ticket back without a call.
 * ifx_segmentation_snapshot_stats: out4 = the tick the ticket pinned (what ifx_tick returned when it was taken), its pixels that name a surfel, how many of those lost their surfel at the
 *   last deferred call (-1: none yet), tickets in use.  Synchronises.  A released ticket's figures stay readable until a new snapshot takes its buffers.
 * Refusals.  IFX_E_INVALID: an unknown or released ticket (_stats: unknown), bad arguments.  IFX_E_STATE, with nothing enqueued and the handle still usable: a sharded
 *   handle (n_ranks > 1 or -1, ifx_set_shard); more than one camera context; no frame processed yet; flags bit 1 on a ticket taken without it; a ticket taken before an
 *   ifx_map_upload, which renumbers the creation numbers (a generation counter on the host detects it).  A deformation (ifx_set_deformation) keeps identities: the ticket
 *   stays valid. */
int ifx_segmentation_snapshot(ifx_t* h, int flags);
int ifx_process_segmentation_deferred(ifx_t* h, int ticket, const uint8_t* masks, const int32_t* class_ids, int n, int frame, int flags);
int ifx_process_segmentation_deferred_device(ifx_t* h, int ticket, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids, int n, int frame, int flags,
                                             void* stream);
int ifx_segmentation_snapshot_release(ifx_t* h, int ticket);
int ifx_segmentation_snapshot_stats(ifx_t* h, int ticket, int32_t* out4);
/* ---- the mask head's own output: ROI masks and boxes, pasted on the device.  A maskrcnn-benchmark / detectron-style mask head yields n x 1 x M x M probabilities
 * (M = 28) and n boxes; the reference's bridge (build/mask_benchmark.py through COCODemo.compute_prediction) turns them into image-sized masks with
 * maskrcnn-benchmark's Masker on the CPU, one mask at a time: paste_mask_in_image with expand_masks and expand_boxes,
 * deps/maskrcnn-benchmark-master/maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py:91-154.  These entries take the n x (M^2 + 4) floats as they are.
 * d_roi_masks: n x M x M f32 (device), contiguous ([N,1,M,M] is the same layout), roi_size = M in 1 .. 64.  d_boxes: n x 4 f32 (device), (x0, y0, x1, y1) in
 * FRAME pixel coordinates.  threshold: a pixel is inside iff its interpolated value is > threshold (the Masker's default 0.5; NaN is outside).
 * The paste rule, every operation rounded to f32 and none fused (S = M + 2):
 *   the ROI mask inside a border of one zero sample (padding = 1); scale = f32(double(S) / M);
 *   wh = (x1 - x0) * 0.5, hh = (y1 - y0) * 0.5, xc = (x1 + x0) * 0.5, yc = (y1 + y0) * 0.5, wh *= scale, hh *= scale;
 *   (b0, b1, b2, b3) = (xc - wh, yc - hh, xc + wh, yc + hh) truncated toward zero to int32;  w = max(b2 - b0 + 1, 1), h = max(b3 - b1 + 1, 1);
 *   sx = f32(S) / f32(w), sy = f32(S) / f32(h);  clip rectangle x in [max(b0, 0), min(b2 + 1, W)), y in [max(b1, 0), min(b3 + 1, H));
 *   per pixel and axis, d = x - b0:  r = max(sx * (f32(d) + 0.5) - 0.5, 0), i0 = min(int(r), S - 1), i1 = min(i0 + 1, S - 1), l1 = r - f32(i0), l0 = 1 - l1;
 *   v = yl0 * (xl0 * pm[yi0][xi0] + xl1 * pm[yi0][xi1]) + yl1 * (xl0 * pm[yi1][xi0] + xl1 * pm[yi1][xi1]);  inside iff v > threshold.
 * Held against the reference's own functions pixel for pixel except where |v - threshold| <= 2^-22 (its vectorised resize fuses multiply-adds):
 * tests/test_roi_paste_cpu.py.  Where the reference raises, the mask is empty and the call goes on: a box with no pixel in the image, a non-finite coordinate,
 * a coordinate beyond +-2^24.  Behind the paste come the bridge's two steps as for ifx_process_segmentation_device (binarise, STABLE sort by area, descending).
 * ifx_process_segmentation_rois: everything else as ifx_process_segmentation_device -- any input order, event wait on `stream`, the resident frame, n <= 256, flags.
 *   Result: bit for bit that of ifx_process_segmentation_device on the n x H x W masks the rule above gives.
 * ifx_process_segmentation_deferred_rois: the deferred call fed the same way; ticket rules as ifx_process_segmentation_deferred_device.
 * ifx_paste_roi_masks: the ingestion alone, as a stage -- what the calls above would hand on.  Downloads, each to a HOST pointer that may be NULL: the 0/255 masks
 *   in the bridge's order (n x H x W), the same after the overlap clean (maskCleanOverlap), the order (n input indices) and the class ids in that order.
 *   Synchronises.  n == 0 writes nothing.
 * Refusals (nothing enqueued, the handle stays usable): IFX_E_INVALID for roi_size outside 1 .. 64, n < 0, n > 256 or NULL device pointers with n > 0;
 * IFX_E_STATE on a sharded handle; the deferred entry refuses as ifx_process_segmentation_deferred_device does. */
int ifx_process_segmentation_rois(ifx_t* h, const float* d_roi_masks, int roi_size, const float* d_boxes, float threshold, const int32_t* d_class_ids, int n, int frame, int flags,
                                  void* stream);
int ifx_process_segmentation_deferred_rois(ifx_t* h, int ticket, const float* d_roi_masks, int roi_size, const float* d_boxes, float threshold, const int32_t* d_class_ids, int n,
                                           int frame, int flags, void* stream);
int ifx_paste_roi_masks(ifx_t* h, const float* d_roi_masks, int roi_size, const float* d_boxes, float threshold, const int32_t* d_class_ids, int n, void* stream, uint8_t* out_ori,
                        uint8_t* out_clean, int32_t* out_order, int32_t* out_class_ids);
/* ---- the detector's input, made on the device from the frame that is already there.  The reference makes it on the CPU: COCODemo.build_transform
 * (deps/maskrcnn-benchmark-master/demo/predictor.py:132-160: ToPILImage, Resize(min_image_size), ToTensor, x255 or channel flip, Normalize), then
 * to_image_list(image, SIZE_DIVISIBILITY) (predictor.py:198-202, maskrcnn_benchmark/structures/image_list.py:29-66) pads it and .to(device) uploads 3 * H' * W' * 4
 * bytes.  These entries write the same floats, bit for bit, from the u8 frame in device memory: planar [1][3][H'][W'] f32.
 * The rule (stated once more, with Pillow's tap arithmetic in full, in instancefusion_amd/host/ifx_detector_prep.hpp; in numpy in tests/detector_input_numpy.py):
 *   Size (Resize.get_size, maskrcnn_benchmark/data/transforms/transforms.py:35-55; f64, Python semantics): size = min_size; with max_size > 0 (<= 0: none), if
 *     f64(max(w,h)) / f64(min(w,h)) * size > max_size then size = (int)rint(max_size * min(w,h) / max(w,h)), half to even.  (w <= h and w == size) or (h <= w and
 *     h == size): kept as it is.  Else w < h: ow = size, oh = (int)(f64(size * h) / w); otherwise oh = size, ow = (int)(f64(size * w) / h).
 *     Padded (image_list.py:54-61): size_divisible = d > 0: W' = ceil(ow / d) * d, H' = ceil(oh / d) * d; d == 0: W' = ow, H' = oh.
 *   Resize: Pillow's 8-bit bilinear resampling (what torchvision's Resize does to a PIL image), 22-bit integer taps, horizontal pass first and then vertical, each
 *     clip8(((1 << 21) + sum v * k) >> 22) per channel with a uint8 intermediate, each skipped when its axis keeps its size.
 *   Float tail, per OUTPUT channel c with source channel s = (flags & IFX_DET_SWAP_RB) ? 2 - c : c: t = f32(byte) / 255.f; with IFX_DET_SCALE_255 t = t * 255.f;
 *     out = (t - mean[c]) / std[c]; every operation rounded to f32, none fused, true divisions (predictor.py:142-145: x255 without a flip, or a flip alone;
 *     transforms.py:86-90: both).  mean / std follow the flip, as T.Normalize is applied behind it.
 *   Padding: samples with x >= ow or y >= oh are 0.0f (to_image_list zero-fills behind the normalisation).
 * ifx_detector_input_size (host only: no handle, no GPU): out4 = ow, oh, W', H' by the size rule above (transforms.py:35-55, image_list.py:54-61).
 * ifx_detector_resize_taps (host only): Pillow's taps of one axis -- first[out_size], count[out_size], coeff[out_size][ksize], zero behind count; returns
 *   ksize = 2 * ceil(max(in / out, 1)) + 1, or IFX_E_INVALID (nothing written) for sizes < 1, NULL pointers or ksize > max_ksize.
 * ifx_detector_input: the frame processed last (ticket < 0: the resident frame slot, also while the next frame is announced and its copy-in under way) or the
 *   frame of a snapshot (a ticket of ifx_segmentation_snapshot taken with flags bit 1; the call orders itself behind the snapshot and does NOT release the ticket).
 *   d_out: out_floats >= 3 * H' * W' floats in device memory.  stream is the CONSUMER's stream (the detector's; NULL = the null stream): the call is enqueue-only on
 *   the handle's main stream -- at entry it records an event on `stream` and lets the main stream wait for it (an earlier forward pass may still read d_out), behind
 *   the kernel it records an event on the main stream and lets `stream` wait for it.  No host synchronisation.  The side stream's next copy-in into the frame slot is
 *   held off behind the read, as for a snapshot.  The tap tables are made on the host and cached in the handle per (w, h, ow, oh).
 * ifx_detector_input_image: the same kernel on any u8 H x W x 3 image in device memory (width x height need not be the handle's), as a stage.
 * Refusals (nothing enqueued, the handle stays usable).  IFX_E_INVALID: NULL pointers, min_size < 1, size_divisible < 0, unknown flag bits, a std entry of 0,
 *   out_floats < 3 * H' * W', an unknown or released ticket, a resize scale above 8 on either axis (an output smaller than an eighth of the frame: this bounds the
 *   taps at 17).  IFX_E_STATE (ifx_detector_input only): no frame processed yet, a ticket taken without its frame, a ticket taken before an ifx_map_upload, a sharded
 *   handle or more than one camera context (as the snapshot entries refuse). */
enum { IFX_DET_SWAP_RB = 1, IFX_DET_SCALE_255 = 2 };
typedef struct ifx_detector_prep { int32_t min_size, max_size, size_divisible, flags; float mean[3], std[3]; } ifx_detector_prep;
int ifx_detector_input_size(int width, int height, const ifx_detector_prep* p, int32_t* out4);
int ifx_detector_resize_taps(int in_size, int out_size, int32_t* first, int32_t* count, int32_t* coeff, int max_ksize);
int ifx_detector_input(ifx_t* h, int ticket, const ifx_detector_prep* p, float* d_out, int64_t out_floats, void* stream);
int ifx_detector_input_image(ifx_t* h, const uint8_t* d_rgb, int width, int height, const ifx_detector_prep* p, float* d_out, int64_t out_floats, void* stream);
/* ---- the detector's two operators of its own.  Between the input above and the ROI masks further up, maskrcnn-benchmark's forward pass is stock tensor algebra
 * except for two operators of its extension module maskrcnn_benchmark._C, which exist as CUDA and CPU sources only: _C.roi_align_forward (csrc/cuda/ROIAlign_cuda.cu,
 * the Pooler of the box and the mask head) and _C.nms (csrc/cuda/nms.cu, the RPN's proposal selection and the box head's per-class loop).  Both f32, inference only.
 * Both calls read and write the caller's device buffers, touch no frame or map state, are enqueue-only on `stream` itself (NULL = the null stream; no host
 * synchronisation) and are allowed on any handle, a sharded one included.  In numpy: tests/detector_ops_numpy.py, held against the reference's CPU operators.
 * ifx_roi_align_forward: d_input [batch][channels][height][width], d_rois n x 5 (batch index, x0, y0, x1, y1), d_out [n][channels][pooled_h][pooled_w].
 *   The rule: the loop of RoIAlignForward (ROIAlign_cuda.cu:65-122, bilinear_interpolate :16-62) in the operation order of ROIAlign_cpu.cpp, every operation
 *   rounded to f32 and none fused:
 *     sw = x0 * scale, sh = y0 * scale, ew = x1 * scale, eh = y1 * scale (no rounding of the ROI); rw = max(ew - sw, 1), rh = max(eh - sh, 1);
 *     bw = rw / pooled_w, bh = rh / pooled_h; grid per axis: sampling_ratio if > 0, else ceil(rh / pooled_h), ceil(rw / pooled_w), per ROI and unbounded
 *     (the cost of an ROI grows with its grid, as in the reference);
 *     sample (iy, ix) of bin (ph, pw): y = (sh + ph * bh) + ((iy + 0.5) * bh) / grid_h, x = (sw + pw * bw) + ((ix + 0.5) * bw) / grid_w;
 *     y < -1, y > height, x < -1 or x > width: the sample contributes +0 (the CUDA kernel's choice);  y <= 0 -> 0, x <= 0 -> 0;
 *     yl = (int)y; yl >= height - 1: yh = yl = height - 1, y = yl, else yh = yl + 1 (x likewise); ly = y - yl, lx = x - xl, hy = 1 - ly, hx = 1 - lx;
 *     val = ((hy * hx * v(yl, xl) + hy * lx * v(yl, xh)) + ly * hx * v(yh, xl)) + ly * lx * v(yh, xh), each weight one product;
 *     acc starts at +0 and adds val with iy outer and ix inner; out = acc / f32(grid_h * grid_w).
 *   The batch index is (int) of the float; outside 0 .. batch - 1 the ROI's outputs are 0 and the input is not read.
 *   Refusals (nothing enqueued, the handle stays usable): IFX_E_INVALID for NULL pointers with n > 0, n < 0, batch / channels / height / width / pooled_h /
 *   pooled_w < 1, sampling_ratio < 0, a non-finite spatial_scale (and sizes beyond the launch: n x ceil(channels / 64) or height x width above 2^31 - 1).
 *   n == 0 succeeds and writes nothing.
 * ifx_nms: d_boxes n x 4 (x0, y0, x1, y1), d_scores n, d_groups NULL or n int32, d_keep n int64, d_count one int32; n <= 8192.
 *   The rule (nms.cu): boxes are visited in descending score, equal scores (-0 == +0) by ascending index, a NaN score behind every number.  A visited box that is
 *   not suppressed is kept and suppresses every later box j of its own group (no groups: one group) with IoU > threshold -- strictly; a NaN IoU suppresses
 *   nothing; a suppressed box suppresses nothing.  IoU, f32 and unfused, max / min as fmaxf / fminf: Sa = (x1 - x0 + 1) * (y1 - y0 + 1);
 *   w = max(min(ax1, bx1) - max(ax0, bx0) + 1, 0), h likewise; inter = w * h; IoU = inter / (Sa + Sb - inter).
 *   Output: the kept indices ascending in d_keep[0 .. count), -1 behind them up to n, count in d_count[0].  With groups = class, one call is the box head's
 *   per-class loop (box_head/inference.py:119-132): the concatenation of the per-group results, sorted by index.
 *   Order (one-block sort in LDS), pair mask (64 x 64 tiles of 64-bit words, upper triangle) and reduction all run on the device.  The scratch (order, sorted
 *   boxes, mask words: 8 MB at the cap) lives in the handle, is allocated by the first call and grown on demand; a call on another stream than the last one
 *   waits for the previous call's event on the device.
 *   Refusals: IFX_E_INVALID for n < 0, n > 8192, NULL pointers (d_groups may be NULL; d_boxes / d_scores / d_keep only with n > 0), a NaN threshold.
 *   n == 0 writes count = 0. */
int ifx_roi_align_forward(ifx_t* h, const float* d_input, int batch, int channels, int height, int width, const float* d_rois, int n, float spatial_scale, int pooled_h,
                          int pooled_w, int sampling_ratio, float* d_out, void* stream);
int ifx_nms(ifx_t* h, const float* d_boxes, const float* d_scores, const int32_t* d_groups, int n, float threshold, int64_t* d_keep, int32_t* d_count, void* stream);
/* ---- the RPN's proposal stage and box decoding.  Between the RPN head and the box head the reference runs RPNPostProcessor.forward_for_single_feature_map
 * (maskrcnn_benchmark/modeling/rpn/inference.py:74-121): about forty stock launches and two host synchronisations per level and image.  ifx_rpn_proposals is that
 * stage for ONE level of ONE image in one call: select, decode, clip, filter, suppress, truncate; the output stays on the device and no count is read back.
 * ifx_box_decode is BoxCoder.decode (modeling/box_coder.py:52-95) alone, which the box head's PostProcessor needs a second time.  Both as the operators above:
 * f32, the caller's buffers on the caller's stream, no frame or map state, any handle.  In numpy: tests/rpn_proposals_numpy.py, held against the reference's
 * own Python through tests/golden/rpn_proposals_ref.npz.
 * ifx_rpn_proposals.  Inputs as the RPN head emits them with N = 1 dropped: d_objectness [A][H][W], d_regression [4A][H][W], d_anchors [H W A][4] (x0, y0, x1, y1) in
 *   the reference's order, anchor a of cell (y, x) at row i = (y W + x) A + a.  permute_and_flatten (rpn/utils.py) is done by indexing: the logit of i is
 *   objectness[a][y][x], its code c is regression[4a + c][y][x].  n = A H W <= 2^24.
 *   Order (inference.py:86-93, topk on the sigmoid): a higher LOGIT first (the sigmoid is monotone), -0 == +0, a NaN behind every number, equal logits by ascending
 *     i -- ifx_nms's order.  The candidates are the first min(pre_nms_top_n, n) in this order.
 *   Decode (box_coder.py:62-93, operation for operation, f32, none fused): w = x1 - x0 + 1, h likewise; cx = x0 + 0.5 w; dx = code0 / wx, dy = code1 / wy (true
 *     divisions); dw = min(code2 / ww, xform_clip), dh likewise, a NaN stays NaN; pcx = dx w + cx; pw = EXP(dw) w; x0' = pcx - 0.5 pw;
 *     x1' = (pcx + 0.5 pw) - 1; y likewise.
 *   EXP is this library's own exponential, no library exp on either side: a NaN gives a NaN; x to f64, clamped into [-104, 90]; k = rint(x * 1.4426950408889634);
 *     r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10; p = the Horner sum of r^i / i! for i = 13 .. 0 in f64 with the coefficients
 *     1.0 / i!, each step p * r + c as a separate multiplication and addition; the result is (float) ldexp(p, k).
 *   Clip (BoxList.clip_to_image, structures/bounding_box.py:214-219): x0', x1' into [0, image_w - 1], y0', y1' into [0, image_h - 1]; a NaN stays NaN.
 *   Small boxes (remove_small_boxes, structures/boxlist_ops.py:34-48): a candidate stays iff x1' - x0' + 1 >= min_size and y1' - y0' + 1 >= min_size (a NaN compares
 *     false); the survivors keep their order.
 *   Suppression (boxlist_nms, boxlist_ops.py:9-31): exactly ifx_nms's rule, one group, on the survivors in the order they have; the first post_nms_top_n kept boxes
 *     in that order are the result.
 *   Output: d_boxes [post_nms_top_n][4], d_logits [post_nms_top_n] (the logits; the reference's "objectness" field is their sigmoid), d_index [post_nms_top_n] int64
 *     (the flat anchor index i), d_count one int32; behind the count boxes and logits are 0 and indices -1.  d_logits and d_index may be NULL.
 *   How: n <= 8192: one block sorts every key in LDS.  Above: a radix select over the key's 32 bits (three multi-block histogram passes, 11 + 11 + 10 bits) finds the
 *     key of rank pre_nms_top_n, ties at it go to the lowest i, a counting pass and a compaction gather the winners, and the same one-block sort orders them.  That
 *     kernel also decodes, clips, filters and compacts; ifx_nms's pair mask and reduction follow, the reduction stopping once post_nms_top_n boxes are kept.
 *     The scratch is ifx_nms's (grown on demand, ordered across streams by its event): no host synchronisation, no allocation on a repeated call of the same size.
 *   Refusals (nothing enqueued, the handle stays usable), IFX_E_INVALID: NULL p, d_boxes or d_count (the inputs only with n > 0), A, H or W < 0, n > 2^24,
 *     pre_nms_top_n or post_nms_top_n outside 1 .. 8192, a NaN nms_thresh, a weight that is 0 or not finite, image_w or image_h < 1.  n == 0 sets the count to 0
 *     and writes the padding.  xform_clip <= 0 or NaN: the reference's default (float) log(1000 / 16).
 * ifx_box_decode: d_codes [n][4k], d_boxes [n][4] -> d_out [n][4k]: the decode above of code j of row r against box r, k = 81 in the box head with the weights
 *   (10, 10, 5, 5); clip_w, clip_h >= 1: the clip above, 0, 0: none.  Refusals: n < 0, k < 1, n k > 2^31 - 1, NULL pointers (the buffers only with n > 0), a weight
 *   that is 0 or not finite, one of clip_w, clip_h 0 and the other not, or one < 0.  n == 0 succeeds and writes nothing. */
typedef struct ifx_rpn_params {
  int32_t pre_nms_top_n, post_nms_top_n;   /* 1 .. 8192 each */
  float   nms_thresh, min_size;
  float   weights[4];                       /* wx, wy, ww, wh; each finite and != 0 */
  float   xform_clip;                       /* <= 0 or NaN: (float)log(1000/16) */
  int32_t image_w, image_h;                 /* >= 1 */
} ifx_rpn_params;
int ifx_rpn_proposals(ifx_t* h, const float* d_objectness, const float* d_regression, const float* d_anchors, int A, int H, int W,
                      const ifx_rpn_params* p, float* d_boxes, float* d_logits, int64_t* d_index, int32_t* d_count, void* stream);
int ifx_box_decode(ifx_t* h, const float* d_codes, const float* d_boxes, int n, int k, const float weights[4], float xform_clip,
                   int clip_w, int clip_h /* 0, 0: no clip */, float* d_out, void* stream);
/* ---- the RPN's proposal stage over all levels of an FPN.  For a model with a feature pyramid the reference runs forward_for_single_feature_map once per level and
 * then RPNPostProcessor.select_over_all_levels (modeling/rpn/inference.py:152-179, the branch that is not training): the levels' results concatenated in ascending
 * level order, topk on the sigmoid, a gather.  ifx_rpn_proposals_fpn is both for ALL levels of ONE image in one call: the per-level stages run side by side in the
 * same launches with the level as a grid dimension, the selection over the levels runs on the device, nothing is read back, and the number of enqueued operations
 * (one memset, at most nine launches) does not depend on the number of levels.  As the operators above: f32, the caller's buffers on the caller's stream, enqueue
 * only, no frame or map state, any handle (a sharded one too).  In numpy: tests/rpn_fpn_numpy.py, held against the reference's own RPNPostProcessor.forward through
 * tests/golden/rpn_fpn_ref.npz.
 *   Inputs: levels: a HOST array of n_levels entries (1 <= n_levels <= 8), each with the device pointers and A, H, W of ifx_rpn_proposals' inputs for that level;
 *     p: the parameters shared by every level.
 *   Per level l = 0 .. L - 1: (boxes_l, logits_l, index_l, c_l) is exactly what ifx_rpn_proposals gives for that level with p: select, decode, clip, small-box
 *     filter, suppression, the cut at post_nms_top_n.  A level with A H W == 0 contributes nothing (c_l = 0).
 *   Selection over the levels: the concatenation in ascending level order has T = sum c_l rows, row r of level l at position off_l + r, off_l = sum of c_l' over
 *     l' < l.  The order: a higher LOGIT first, -0 == +0, a NaN behind every number, equal logits by ascending position -- ifx_nms's order on (logit, position).
 *     The result is the first min(fpn_post_nms_top_n, T) rows in that order.  The reference orders by the sigmoid, which is monotone but not injective in f32, and
 *     torch's topk does not define the order among equal values: this rule is one of the results the reference permits, fixed.
 *   Output, F = fpn_post_nms_top_n: d_boxes [F][4], d_logits [F] (the logits; the reference's "objectness" field is their sigmoid), d_level [F] int32 (l),
 *     d_index [F] int64 (the flat anchor index i inside its level), d_count one int32 = min(F, T), d_level_counts [n_levels] int32 (c_l).  Behind the count boxes and
 *     logits are 0, level and index -1.  d_logits, d_level, d_index and d_level_counts may be NULL.  T == 0 writes the padding and the count 0.  There is no cap
 *     on T.
 *   How: a table of the levels (pointers, sizes, each level's slices of the scratch, every slice sized from the level's own min(pre_nms_top_n, n)) travels by value
 *     in the kernel arguments.  The radix select's five kernels take the level from blockIdx.y (blocks of a level with n <= 8192 leave at once; with no such level
 *     the memset and the five launches are skipped); one 1024-thread block per level sorts, decodes and filters; one launch computes every level's pair mask; one
 *     block per level walks its mask up to post_nms_top_n kept rows and writes the level's kept list.  Every list is already in the rule's order, so the selection
 *     needs no sort: a row's rank is its row number plus, per other level, the number of that level's rows in front of it (a binary search with the 64-bit key
 *     (logit key, position)); the ranks are a permutation of 0 .. T - 1 and rank < F writes its output row.  The scratch is ifx_nms's: no allocation on a repeated
 *     call of the same sizes.
 *   Refusals (nothing enqueued, the handle stays usable), IFX_E_INVALID: n_levels outside 1 .. 8; fpn_post_nms_top_n outside 1 .. 8192; NULL levels, p, d_boxes
 *     or d_count; a level with NULL inputs and n > 0; a negative A, H or W; a level with n > 2^24; everything ifx_rpn_proposals refuses in p. */
typedef struct ifx_rpn_level { const float *objectness, *regression, *anchors; int32_t A, H, W; } ifx_rpn_level;   /* as ifx_rpn_proposals' inputs */
int ifx_rpn_proposals_fpn(ifx_t* h, const ifx_rpn_level* levels, int n_levels, const ifx_rpn_params* p, int fpn_post_nms_top_n,
                          float* d_boxes, float* d_logits, int32_t* d_level, int64_t* d_index, int32_t* d_count, int32_t* d_level_counts, void* stream);
/* ---- the box head's post-processing.  Behind the box head the reference runs PostProcessor.forward with filter_results (maskrcnn_benchmark/modeling/roi_heads/
 * box_head/inference.py:43-146): a softmax, BoxCoder.decode over [R, 4 C], a clip, then a Python loop over the classes with a nonzero, two gathers and boxlist_nms
 * each, and a kthvalue on the host -- about 160 host round trips per image.  ifx_box_detections is that stage for ONE image in one call: class logits, box
 * regression and proposals in, final boxes, scores, labels and proposal rows out; enqueue only, nothing is read back.  As the operators above: f32, the caller's
 * buffers on the caller's stream, no frame or map state, any handle (a sharded one too).  In numpy: tests/box_detections_numpy.py, held against the reference's
 * own Python through tests/golden/box_detections_ref.npz.
 *   Inputs: d_logits [R][C]; d_regression [R][4 Creg], Creg == C, or Creg == 1 (cls_agnostic_bbox_reg: the code of every class is columns 0 .. 3; the caller has
 *     taken the reference's [:, -4:] slice); d_proposals [R][4] (x0, y0, x1, y1).  2 <= C <= 1024, R >= 0, R C <= 2^24.
 *   Softmax (F.softmax(class_logits, -1)), per row: m = the row's maximum in f32.  A NaN in the row, or m not finite: every probability of the row is NaN and the
 *     row yields no candidate (torch gives NaNs for the whole row).  Otherwise d_j = x_j - m rounded to f32; e_j = EXP(d_j), the exponential of ifx_rpn_proposals
 *     above (e at the maximum is exactly 1); s = sum_j (double) e_j in f64 with j ascending from 0, each addition rounded once -- the order is part of the rule;
 *     p_j = (float) ((double) e_j / s).  Against exp(d_j) / sum exp(d_i) in f64 the golden cases' probabilities are within 1.443 ulp (bound 3: one rounding each
 *     from EXP, s and the conversion); torch's CPU softmax reaches 3.224 ulp there, and the two differ by at most 4.000 ulp.
 *   Candidates: the pairs (r, j), j = 1 .. C - 1, with p[r][j] > score_thresh (strictly; a NaN compares false).  The box of a candidate: the decode of code j (code 0
 *     with Creg == 1) of row r against proposal r with the given weights and xform_clip, clipped to image_w x image_h -- decode and clip as stated for
 *     ifx_rpn_proposals.  Candidate order is class-major: j ascending, r ascending within a class (the order of the reference's concatenation).  K = their number.
 *   Overflow: K > 8192: the call writes the padding only, d_count[0] = -1 and d_stats = {K, 0}.  The reference has no such cap; a caller meets it by raising
 *     score_thresh (with the released 0.05 a row gives at most 19 candidates; K is typically in the hundreds).
 *   Suppression: ifx_nms's rule with group = class on the candidates, threshold nms: visited by descending score, equal scores by ascending candidate position.
 *     D = the number kept; the kept candidates stay in candidate order (boxlist_nms returns ascending indices per class, cat_boxlist concatenates by class).
 *   Limit (inference.py:137-145): detections_per_img = M > 0 and D > M: t = the M-th largest kept score; every kept candidate with score >= t stays, in candidate
 *     order.  Ties at t all stay: the result can exceed M, as in the reference.  M <= 0: no limit.
 *   Output: d_boxes [max_out][4], d_scores [max_out] (the probabilities), d_labels [max_out] int64 (j), d_index [max_out] int64 (the proposal row r), d_count one
 *     int32, d_stats two int32 {K, D}; d_scores, d_labels, d_index and d_stats may be NULL.  d_count[0] is the number the rule keeps -- it may exceed max_out (ties,
 *     or M <= 0); the first min(count, max_out) detections are written, behind them boxes and scores are 0, labels and indices -1.
 *   How: one wave per row for the softmax (every lane runs the same ascending f64 sum out of LDS) writing p, or a NaN for "no candidate", into a class-major plane;
 *     per-block counts and a scan compact the candidates in class-major order without atomics that could show, K stays on the device; one block sorts the
 *     candidates (ifx_nms's network) and decodes and clips each one's box; ifx_nms's pair mask with groups; one block walks the mask, finds t at the M-th kept row
 *     of the sorted order, moves the flags to candidate order and writes the outputs.  The scratch is ifx_nms's (grown on demand, ordered across streams by its
 *     event): no host synchronisation, no allocation on a repeated call of the same size.
 *   Refusals (nothing enqueued, the handle stays usable), IFX_E_INVALID: NULL p, d_boxes or d_count; NULL inputs with R > 0; R < 0, C outside 2 .. 1024,
 *     R C > 2^24, Creg not in {1, C}; max_out outside 1 .. 8192, detections_per_img > max_out; a NaN score_thresh or nms; a weight that is 0 or not finite; image_w
 *     or image_h < 1.  R == 0 writes count 0, stats {0, 0} and the padding.  xform_clip <= 0 or NaN: the default, as above. */
typedef struct ifx_box_det_params {
  float   score_thresh, nms;                /* neither a NaN */
  int32_t detections_per_img;               /* M; <= 0: no limit; <= max_out */
  int32_t max_out;                          /* 1 .. 8192: the rows of the output buffers */
  float   weights[4];                       /* wx, wy, ww, wh; each finite and != 0 */
  float   xform_clip;                       /* <= 0 or NaN: (float)log(1000/16) */
  int32_t image_w, image_h;                 /* >= 1 */
} ifx_box_det_params;
int ifx_box_detections(ifx_t* h, const float* d_logits, const float* d_regression, const float* d_proposals, int R, int C, int Creg,
                       const ifx_box_det_params* p, float* d_boxes, float* d_scores, int64_t* d_labels, int64_t* d_index, int32_t* d_count,
                       int32_t* d_stats, void* stream);
/* ---- multi-level ROI pooling.  In front of the box head and of the mask head the reference runs the FPN Pooler (maskrcnn_benchmark/modeling/poolers.py:11-121):
 * LevelMapper in about ten stock launches, then per level a nonzero (a host synchronisation), a gather, _C.roi_align_forward and an index_put into a zero-filled
 * result.  ifx_fpn_roi_align is Pooler.forward behind convert_to_roi_format in ONE launch: every block finds its ROI's level and runs ifx_roi_align_forward's body
 * against that level's map.  As the operators above: f32, the caller's buffers on the caller's stream, enqueue only, no scratch, no allocation, no frame, map or
 * handle state, any handle (a sharded one too).  In numpy: tests/fpn_pooler_numpy.py, held against the reference's own Pooler.forward and LevelMapper through
 * tests/golden/fpn_pooler_ref.npz.
 *   Inputs: d_features, heights, widths, scales: HOST arrays of `levels` entries (1 <= levels <= 8), d_features[l] the device pointer of level l's map
 *     [batch][channels][heights[l]][widths[l]]; d_rois n x 5 (batch index, x0, y0, x1, y1); d_out [n][channels][pooled_h][pooled_w]; d_levels NULL or n int32.
 *   Scales: scales[l] == 2^-(k_min + l) exactly, for an integer k_min >= 0 (the Pooler's own assumption, poolers.py:72-76: its k_min and k_max are -log2 of the
 *     first and the last scale); k_max = k_min + levels - 1 <= 126.
 *   Level of an ROI (LevelMapper, poolers.py:31-42, with BoxList.area, structures/bounding_box.py:226-236), every operation rounded to f32 and none fused:
 *     area = (x1 - x0 + 1) * (y1 - y0 + 1);  s = sqrt(area), correctly rounded;  v = s / canonical_scale + eps (a true division; defaults 224 and 1e-6f);
 *     L = log2(v) evaluated in f64 and rounded once to f32;  t = f32(canonical_level + L) (default 4);  level = clamp(floor(t), k_min, k_max) - k_min.
 *     The two roundings of L and t are part of the rule: just below a power of two, canonical_level + L rounds up to the integer, as torch.floor(4 + torch.log2(v))
 *     does on the CPU.  A NaN t -- a negative or NaN area (a non-finite coordinate), or a v < 0, which only a negative eps can give -- is NO level: the ROI's outputs
 *     are zeros, no map is read and d_levels is -1 (the reference's `levels == level` never matches it, so its row of the zero-filled result stays).  An area of 0
 *     goes to level 0, +inf to the last level.
 *     How: the level is monotone in v, so the host finds per call the levels - 1 thresholds T_j = the smallest f32 v >= 0 whose rule value reaches level j, by
 *     bisection over f32 bit patterns with the host's f64 log2, and passes them by value with the level table; on the device one lane computes v (a correctly
 *     rounded square root, an IEEE division, an addition), counts the T_j that v reaches and hands the level to its block through LDS.
 *     ifx_fpn_level_thresholds (host only, no handle): out[j - 1] = T_j for j = 1 .. levels - 1; returns k_min, or IFX_E_INVALID for NULL pointers, levels outside
 *     1 .. 8 or scales that are not the ladder.
 *   levels == 1: no mapping at all (poolers.py:101-102): the call is ifx_roi_align_forward on that map, NaN-area ROIs included, and d_levels is 0.
 *   Pooling: ifx_roi_align_forward's rule with the level's map, height, width and scale; the batch rule too (an index outside 0 .. batch - 1: zeros).
 *   d_levels (optional) receives the level index of every ROI, -1 for no level.
 *   Refusals (nothing enqueued, the handle stays usable), IFX_E_INVALID: levels outside 1 .. 8; NULL d_features, heights, widths, scales or an entry of d_features;
 *     NULL d_rois or d_out with n > 0; n < 0, batch / channels / a height / a width / pooled_h / pooled_w < 1, sampling_ratio < 0; scales that are not the ladder;
 *     a canonical_scale that is not a positive finite number; a non-finite eps; sizes beyond the launch, as ifx_roi_align_forward.  n == 0 succeeds and writes
 *     nothing. */
int ifx_fpn_level_thresholds(const float* scales, int levels, int canonical_level, float* out);
int ifx_fpn_roi_align(ifx_t* h, const float* const* d_features, const int32_t* heights, const int32_t* widths, const float* scales, int levels, int batch, int channels,
                      const float* d_rois, int n, float canonical_scale, int canonical_level, float eps, int pooled_h, int pooled_w, int sampling_ratio, float* d_out,
                      int32_t* d_levels, void* stream);
/* ---- the mask head's logits to the map's votes: select, sigmoid, paste.  Between the mask head's last convolution and the map the reference runs
 * MaskPostProcessor.forward (maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py:27-61: a sigmoid over all [R, C, M, M] logits of which C - 1 of every C
 * are thrown away, an arange and an advanced-index gather), prediction.resize((width, height)) (demo/predictor.py:213 with BoxList.resize, structures/
 * bounding_box.py:91-127) and COCODemo.select_top_predictions (demo/predictor.py:224-243: a compare, a nonzero that makes the host wait, a gather of every field,
 * a sort by score and a second gather); the bridge (build/mask_benchmark.py:54-82) then sorts the pasted masks by area.  ifx_mask_head_select is that stretch for
 * ONE image in two launches, ifx_process_segmentation_detections runs it in front of ifx_process_segmentation_rois.  In numpy: tests/mask_head_numpy.py, held
 * against the reference's own Python through tests/golden/mask_head_ref.npz (tests/test_mask_head_cpu.py).
 *   Inputs: d_mask_logits [R][C][M][M] f32; d_boxes [R][4] f32 (x0, y0, x1, y1) in the coordinates of the network's input, BoxList.size = (in_w, in_h);
 *     d_scores [R] f32; d_labels [R] int64, as ifx_box_detections emits them; d_count one int32 on the device or NULL: the valid rows are the first
 *     min(max(count, 0), R), NULL: all R (a padded ifx_box_detections result goes in without a read-back); d_class_map int32 [C] on the device or NULL: the class id
 *     handed on for label j, NULL: the label itself.  1 <= M <= 64, 1 <= C <= 1024, 0 <= R <= 1024.
 *   Kept rows: a valid row r is kept iff scores[r] > score_thresh (strictly; a NaN score compares false) and 0 <= labels[r] < C.  The reference would raise on a
 *     label outside the range; here the row is dropped.  score_thresh == -inf: the score is not examined at all and every valid row with a good label is kept, a
 *     score of -inf or NaN too -- MaskPostProcessor.forward, which has no score test.  A NaN score_thresh is refused.
 *   Order: sort_by_score != 0: select_top_predictions' -- a higher score first, -0 == +0, equal scores by ascending row (a NaN, which only score_thresh == -inf
 *     lets through, behind every number): ifx_nms's key order and its sort network.  torch's descending sort is not stable: among equal scores this rule is one of
 *     the orders the reference permits, fixed.  sort_by_score == 0: ascending row, a stable compaction -- MaskPostProcessor's own order.
 *   Boxes (BoxList.resize): rw = (float)((double)out_w / (double)in_w), rh likewise; x' = x * rw, y' = y * rh, one f32 multiplication each.  The reference forms
 *     the ratios as Python floats and multiplies the f32 tensor by them -- `bbox * ratio` when the two ratios are equal, per-coordinate products otherwise; torch
 *     rounds the scalar to f32 before the multiplication on both branches.  Held bit for bit against BoxList.resize on the CPU for equal and unequal ratios.
 *   Probabilities: only the kept row's own channel is read: x = logits[r][labels[r]][y][x];  e = EXP(-x), d = 1.0f + e, p = 1.0f / d, each step rounded to f32,
 *     none fused, a true division; EXP is the exponential stated under ifx_rpn_proposals.  A NaN gives a NaN, which the paste treats as outside.  EXP's clamp makes
 *     p exactly 1 far to the right (EXP(-x) rounds to +0 from x = 104 on, and 1 + e rounds to 1 long before; +inf too) and exactly 0 far to the left (EXP(-x)
 *     overflows to +inf below x = -88.8; -inf too).  Against torch's CPU sigmoid the golden cases' samples
 *     differ by at most 1.192093e-07 (2.000 ulp of torch's value): measured by tools/make_golden_mask_head.py, which writes the figures here and into the fixture.
 *   Output, R rows each: d_roi_masks [R][M][M], d_boxes_out [R][4], d_class_ids [R] int32, d_rows [R] int32 (the input row of each kept detection; may be NULL),
 *     d_kept one int32.  Behind kept, masks and boxes are 0, class ids and rows -1.
 *   How: one block of 1024 threads, one thread per row, reads the count from the device, tests the row, scans (the detector operators' block scan) and, with
 *     sort_by_score, sorts the keys in LDS; thread k then writes output row k -- the resized box, the class id, the row -- or the padding.  One launch of R blocks
 *     follows: block k leaves after writing zeros if k >= kept, otherwise it reads the M^2 logits of (rows[k], label) and writes the M^2 probabilities.  The row
 *     travels from the first launch to the second in the first word of the output mask it belongs to, so a NULL d_rows needs no scratch.
 * ifx_mask_head_select: the stage on the caller's buffers and stream: enqueue only, no host synchronisation, no allocation, no frame or map state, any handle (a
 *   sharded one too).  R == 0 writes kept = 0 and nothing else.
 * ifx_process_segmentation_detections: the stage into scratch of the handle (the detector operators' buffer, grown on demand: a repeated call of the same size
 *   allocates nothing) on `stream`, the producer's, with out_w x out_h = the handle's frame size (the struct's out_w, out_h are ignored); one 4-byte read of kept,
 *   the only wait the call adds in front of the one at its end; then exactly ifx_process_segmentation_rois on the kept ROI masks, boxes and class ids with
 *   `threshold` (the Masker's, 0.5), frame and flags.  *out_kept (host, may be NULL) receives kept.  kept > 256: IFX_E_CAPACITY, nothing is applied, the handle
 *   stays usable.  kept == 0 is the ROI entry's n == 0.  The result is bit for bit that of ifx_process_segmentation_rois fed the stage's outputs.
 * ifx_process_segmentation_deferred_detections: the same behind a snapshot ticket; ticket rules as ifx_process_segmentation_deferred_rois (a call that fails,
 *   IFX_E_CAPACITY included, keeps the ticket).
 * Refusals (nothing enqueued, the handle stays usable): IFX_E_INVALID for M, C or R outside their ranges, NULL p, d_kept or output buffers, NULL inputs with
 *   R > 0, a NaN score_thresh, in_w, in_h, out_w or out_h < 1 (out_w, out_h: the stage entry only); IFX_E_STATE on a sharded handle for the two process entries;
 *   the deferred entry refuses as ifx_process_segmentation_deferred_rois does. */
typedef struct ifx_mask_head_params {
  float   score_thresh;                     /* not a NaN; -inf: no score test */
  int32_t in_w, in_h;                       /* >= 1: the size the boxes are given in */
  int32_t out_w, out_h;                     /* >= 1: the size they are resized to */
  int32_t sort_by_score;                    /* != 0: select_top_predictions' order; 0: ascending row */
} ifx_mask_head_params;
int ifx_mask_head_select(ifx_t* h, const float* d_mask_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels, const int32_t* d_count,
                         const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, float* d_roi_masks, float* d_boxes_out,
                         int32_t* d_class_ids, int32_t* d_rows, int32_t* d_kept, void* stream);
int ifx_process_segmentation_detections(ifx_t* h, const float* d_mask_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels,
                                        const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, float threshold,
                                        int frame, int flags, void* stream, int32_t* out_kept);
int ifx_process_segmentation_deferred_detections(ifx_t* h, int ticket, const float* d_mask_logits, const float* d_boxes, const float* d_scores,
                                                 const int64_t* d_labels, const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M,
                                                 const ifx_mask_head_params* p, float threshold, int frame, int flags, void* stream, int32_t* out_kept);
/* ---- the reference's default detector (IF/main.cpp:33, maskRcnnType = 1 -> build/mask_ori.py: the Keras Mask R-CNN under deps/mask_rcnn).  Its model ends in
 * detections [R,6] and mrcnn_mask [R,M,M,C]; MaskRCNN.unmold_detections (deps/mask_rcnn/model.py:2285-2344) turns them into image-sized masks on the CPU, one
 * detection at a time, through utils.unmold_mask (deps/mask_rcnn/utils.py:490-507) and scipy.misc.imresize: a per-mask min/max stretch to bytes, Pillow's 8-bit
 * bilinear resampling to the box's size, a threshold, a paste.  ifx_unmold_detections is that routine for ONE image on the device; ifx_process_segmentation_unmolded
 * runs it in front of ifx_process_segmentation_device.  In numpy: tests/unmold_numpy.py, held against the reference's own Python through
 * tests/golden/unmold_cases.npz (tests/test_unmold_cpu.py).
 *   Inputs: d_detections [R][6] f32 (y1, x1, y2, x2, class_id, score) in molded-image pixels, zero rows behind the last detection; d_masks f32, [R][M][M][C]
 *     (IFX_UNMOLD_NHWC, as Keras emits it) or [R][C][M][M] (IFX_UNMOLD_NCHW); window[4] int32 ON THE HOST (wy1, wx1, wy2, wx2), the image's place in the molded
 *     input (ifx_molded_input_size's last four); d_class_map int32 [C] on the device or NULL, as ifx_mask_head_select takes it; width x height: the image the
 *     masks are made for.  0 <= R <= 1024, 1 <= M <= 64, 2 <= C <= 1024.  Every f32 operation is rounded to f32, none is fused.
 *   1 Count: N = the first row with class_id == 0.0f (-0 too), R when there is none (model.py:2304-2305).
 *   2 Boxes (model.py:2314-2322): scale = min(height / (wy2 - wy1), width / (wx2 - wx1)) on the host in f64; per coordinate k with the shift (wy1, wx1, wy1, wx1):
 *     b_k = (int32)trunc((f64(det[k]) - f64(shift_k)) * scale) -- numpy promotes f32 - int64 to f64.
 *   3 Exclusion (model.py:2326-2333): a row survives iff (y2 - y1) * (x2 - x1) > 0, in int64.  Dropped rows vanish, later rows move up.
 *   4 Bytes (scipy.misc.bytescale behind imresize): c = (int32)class_id, m = the M x M samples of channel c of the row; cmin, cmax over them; cs = f32(cmax - cmin),
 *     1 if that is 0; s = f32(255.0 / f64(cs)); byte = (uint8)trunc(min(max(f32(f32(m - cmin) * s), 0), 255) + 0.5f).  This is bytescale as numpy evaluated it
 *     when the reference was written: float / np.float32 gave a float64 scalar, and a float64 scalar did not widen a float32 array.
 *   5 Resize: the M x M bytes to h = y2 - y1 rows and w = x2 - x1 columns by the 8-bit rule stated under ifx_detector_input: the taps of precompute_coeffs with
 *     in = M in f64 (PRECISION_BITS 22), made on the device per detection and equal to ifx_detector_resize_taps' integer for integer; the horizontal pass first,
 *     a uint8 intermediate [M][w], then the vertical pass; each pass clip8((2^21 + sum v * k) >> 22), an axis that keeps the size M being the identity.
 *   6 Threshold: inside iff the byte >= 128 (f32(b) / 255.0f >= 0.5f holds exactly from 128 on).  7 Paste: pixel (y1 + j, x1 + i) (utils.py:505-506).
 *   8 Where the reference raises or has no defined result the row's mask is empty and the call goes on (the ROI entry's convention); the row still counts:
 *     a box not within 0 <= y1 < y2 <= height, 0 <= x1 < x2 <= width (both extents negative passes step 3); a coordinate that is not finite or beyond +-2^24,
 *     before or after the scale -- such a row skips step 3 and its box is written as zeros; a class id that is NaN or outside 1 .. C - 1 -- its class id is
 *     written as 0, not mapped; a NaN or +-inf among the M^2 samples, or cs or s not finite in f32.
 *   Output, the surviving rows in input order: d_masks_out [R][height * width] u8, 0 / 1; d_class_ids [R] int32 (through d_class_map if given); d_boxes_out
 *     [R][4] int32 (y1, x1, y2, x2); d_scores_out [R] f32 (may be NULL); d_rows [R] int32, the input row (may be NULL); d_kept one int32.  Behind kept: masks,
 *     boxes and scores 0, class ids and rows -1.
 *   How: one block of 1024 threads, one thread per row, does steps 1 to 3 and the detector operators' block scan, and scatters the records; one memset of the
 *     masks; a launch over (column tiles of 64 pixels, R): a block finds its row by the same scan (the box is known only on the device, so nothing travels between
 *     the launches), leaves when it is past kept or beside the box, reduces min / max, stretches the channel to bytes in LDS, makes the horizontal taps of its
 *     columns (one lane per column, f64), resamples into an [M][64] byte tile, then walks the box's rows in chunks of 64 (one lane making one row's taps).
 * ifx_unmold_detections: the stage on the caller's buffers and stream: enqueue only, no host synchronisation, no allocation, no frame or map state, any handle (a
 *   sharded one too; the u8 masks fit ifx_owner_process_segmentation_device).  R == 0 writes kept = 0 and nothing else.
 * ifx_process_segmentation_unmolded: the stage into scratch of the handle (the detector operators' buffer, grown on demand) on `stream`, the producer's, at the
 *   handle's frame size; one 4-byte read of kept, the only wait the call adds; then exactly ifx_process_segmentation_device on the kept masks with IFX_MASK_U8 --
 *   the bridge's maskOri == 1 -> 255 and its stable area sort (build/mask_ori.py:104-117) are that entry's ingestion.  *out_kept (host, may be NULL) receives
 *   kept; kept == 0 is n == 0.  R > 256 is refused: the scratch is R x P bytes, and the reference's R is 100 (DETECTION_MAX_INSTANCES, deps/mask_rcnn/config.py).
 * ifx_process_segmentation_deferred_unmolded: the same behind a snapshot ticket; ticket rules as ifx_process_segmentation_deferred_device.
 * Refusals (nothing enqueued, the handle stays usable, ifx_last_error starts with the entry's name): IFX_E_INVALID for R, M or C outside their ranges, an
 *   unknown layout, NULL inputs or outputs with R > 0, a NULL window or d_kept, a window with wy2 <= wy1 or wx2 <= wx1, width or height < 1 (the stage), R > 256
 *   (the process entries); IFX_E_STATE on a sharded handle for the process entries. */
enum { IFX_UNMOLD_NHWC = 0, IFX_UNMOLD_NCHW = 1 };
int ifx_unmold_detections(ifx_t* h, const float* d_detections, const float* d_masks, const int32_t* window, const int32_t* d_class_map, int R, int M, int C,
                          int layout, int width, int height, uint8_t* d_masks_out, int32_t* d_class_ids, int32_t* d_boxes_out, float* d_scores_out,
                          int32_t* d_rows, int32_t* d_kept, void* stream);
int ifx_process_segmentation_unmolded(ifx_t* h, const float* d_detections, const float* d_masks, const int32_t* window, const int32_t* d_class_map, int R, int M,
                                      int C, int layout, int frame, int flags, void* stream, int32_t* out_kept);
int ifx_process_segmentation_deferred_unmolded(ifx_t* h, int ticket, const float* d_detections, const float* d_masks, const int32_t* window,
                                               const int32_t* d_class_map, int R, int M, int C, int layout, int frame, int flags, void* stream, int32_t* out_kept);
/* ---- the same detector's input: MaskRCNN.mold_inputs (deps/mask_rcnn/model.py:2247-2283) = utils.resize_image (deps/mask_rcnn/utils.py:384-432) + mold_image
 * (model.py:2524-2529): a resize by its own size rule, a centred zero padding to max_dim x max_dim, the mean subtracted without a division, channels last.
 * ifx_molded_input_size (host only: no handle, no GPU), all in f64 with Python's semantics: s = max(1, min_dim / min(h, w)) when min_dim > 0, else 1; if
 *   rint(max(h, w) * s) > max_dim then s = max_dim / max(h, w); nh = rint(h * s), nw = rint(w * s), half to even (Python 3's round; no resize when s == 1);
 *   S = max_dim, top = (S - nh) / 2, left = (S - nw) / 2 by floor division.  out8 = nw, nh, S, S, top, left, top + nh, left + nw -- the last four are the window
 *   ifx_unmold_detections needs.  IFX_E_INVALID: a NULL out8, width or height < 1, max_dim < 1, nh or nw outside 1 .. S, a resize scale above 8 on an axis.
 * ifx_detector_input_molded / _image: the frame sources, the event protocol with the consumer's `stream`, the cached tap tables, the kernel's two resampling
 *   phases and the refusals of ifx_detector_input / _image.  They write S x S x 3 floats: inside the window the Pillow-resized byte b of channel c (RGB order, no
 *   flip) as f32(f64(b) - mean[c]) -- mold_image subtracts an f64 array from an f32 one and Keras casts to f32: one rounding --, in the padding f32(0.0 - mean[c])
 *   (resize_image pads with 0 before the mean is subtracted; +0 for a mean of 0).  mean: double[3] (MEAN_PIXEL, deps/mask_rcnn/config.py).  layout: [S][S][3] (IFX_MOLD_NHWC, Keras)
 *   or [3][S][S] (IFX_MOLD_NCHW).  IFX_E_INVALID also for a NULL mean, an unknown layout and out_floats < 3 * S * S. */
enum { IFX_MOLD_NHWC = 0, IFX_MOLD_NCHW = 1 };
int ifx_molded_input_size(int width, int height, int min_dim, int max_dim, int32_t* out8);
int ifx_detector_input_molded(ifx_t* h, int ticket, int min_dim, int max_dim, const double* mean, int layout, float* d_out, int64_t out_floats, void* stream);
int ifx_detector_input_molded_image(ifx_t* h, const uint8_t* d_rgb, int width, int height, int min_dim, int max_dim, const double* mean, int layout, float* d_out,
                                    int64_t out_floats, void* stream);
/* ---- the same detector's three layers that are no convolutions (deps/mask_rcnn/model.py): ProposalLayer.call (:227-311), PyramidROIAlign.call (:323-424) and
 * DetectionLayer / refine_detections_graph (:670-807) with the box conversion behind it (:1961-1963).  In TensorFlow they are graphs of top_k, gather,
 * non_max_suppression, crop_and_resize, where, unique, map_fn and set_intersection; here each is one enqueue-only call on the caller's buffers and `stream` (NULL =
 * the handle's main stream): no wait for the device, no allocation in steady state (the detector operators' scratch, grown on demand), no frame or map state, the
 * counts stay on the device.  In numpy: tests/keras_layers_numpy.py; TensorFlow's kernels are not in the reference tree, so only utils.apply_box_deltas,
 * utils.non_max_suppression and the level expression are held against executed reference code (tests/golden/keras_layers_ref.npz, tests/test_keras_layers_cpu.py).
 * Common: boxes are y1, x1, y2, x2 with the far corner OUTSIDE (no + 1 anywhere).  All arithmetic is f32, every operation rounded, none fused, divisions true,
 *   sqrt correctly rounded.  EXP is the EXP of ifx_rpn_proposals.  The order of scores is ifx_nms's: descending, -0 == +0, equal scores by ascending index, a NaN
 *   behind every number.
 *   DECODE(box, d), apply_box_deltas_graph (model.py:185-206): h = y2 - y1; w = x2 - x1; cy = y1 + 0.5f h; cx = x1 + 0.5f w; cy += d0 h; cx += d1 w; h *= EXP(d2);
 *     w *= EXP(d3); y1 = cy - 0.5f h; x1 = cx - 0.5f w; y2 = y1 + h; x2 = x1 + w.
 *   CLIP(v, lo, hi), clip_boxes_graph (model.py:209-224): max(min(v, hi), lo) as (v > hi ? hi : v), then (v < lo ? lo : v); a NaN stays a NaN.
 *   TFNMS(boxes in their order, threshold, limit), tf.image.non_max_suppression: per box ymin = min(y1, y2), ymax = max(y1, y2), likewise x (fminf / fmaxf),
 *     area = (ymax - ymin) * (xmax - xmin).  IoU of a pair: 0 if either area <= 0; else inter = max(min(ymax) - max(ymin), 0) * max(min(xmax) - max(xmin), 0) and
 *     iou = inter / (area_a + area_b - inter).  Walking the boxes in order, a box is kept unless a kept box in front of it has iou > threshold with it (strictly; a
 *     NaN compares false); the walk ends when `limit` boxes are kept.
 * ifx_keras_proposals, one image: d_rpn_probs [n][2] (background, foreground), d_rpn_bbox [n][4] deltas, d_anchors [n][4] in PIXELS (ProposalLayer's
 *   self.anchors; utils.generate_pyramid_anchors stays the caller's, constant per configuration).
 *   1 score[i] = probs[i][1], read in place with a stride of two.  2 K = min(pre_nms_limit, n); the K best anchors by the order above (tf.nn.top_k: equal scores
 *   by ascending index).  3 d = bbox[i] * std_dev, per component; box = DECODE(anchor, d).  4 CLIP to 0 .. image_h (y) and 0 .. image_w (x).  5 Divide by
 *   image_h (y) and image_w (x).  6 TFNMS(the K boxes in the selected order, nms_threshold, proposal_count).
 *   Output: d_proposals [proposal_count][4], the kept boxes -- normalised, as decoded, NOT corner-ordered -- in kept order, zero rows behind them; d_index
 *   [proposal_count] int64 (may be NULL), their anchor indices, -1 behind them; d_count one int32, the number kept.
 *   How: n > 8192: one memset, the radix select's five launches with the score's stride as a template argument; then one block sorts and decodes, the pair mask
 *   in its TF form, the walk: eight launches at any n, three when n <= 8192.  The reference's configuration: n = 65 472, K = 6000, 1000 out.
 *   IFX_E_INVALID (nothing enqueued, the handle stays usable): pre_nms_limit or proposal_count outside 1 .. 8192, n outside 1 .. 2^24 - 1, a NULL pointer other
 *   than d_index, image_h or image_w < 1.
 * ifx_pyramid_level_thresholds (host only: no handle, no GPU): out3 = T0, T1, T2 with c = 224 / sqrt(image_h * image_w), T0 = c 2^-1.5, T1 = c 2^-0.5,
 *   T2 = c 2^0.5, computed in f64 and rounded once to f32.  IFX_E_INVALID: a NULL out3 or a size < 1.
 * ifx_pyramid_roi_align: d_features[4], the maps P2 .. P5 of heights[l] x widths[l], [batch][C][H_l][W_l] (layout 0) or [batch][H_l][W_l][C] (layout 1, as Keras
 *   holds them); d_boxes [batch][n][4] normalised; the image of row r is r / n.
 *   Level: s = sqrtf((y2 - y1) * (x2 - x1)); level = 2 + (s > T0) + (s >= T1) + (s > T2).  This is the reference's min(5, max(2, 4 + round(log2(s / c)))) with
 *     tf.round's half-to-even written as compares (-1.5 -> -2, -0.5 -> 0, 0.5 -> 0), so that no device logarithm decides an integer; s zero or NaN: level 2, where
 *     TensorFlow's clamp puts the zero-padded rows.
 *   Sample, tf.image.crop_and_resize(method "bilinear", extrapolation_value 0) on the level's map H x W: for output row i, pool_h > 1: scale = ((y2 - y1) *
 *     (H - 1)) / (pool_h - 1), in_y = y1 * (H - 1) + i * scale; pool_h == 1: in_y = (0.5f * (y1 + y2)) * (H - 1); x likewise with W and pool_w.  in_y < 0,
 *     in_y > H - 1 or NaN (likewise x): 0 for every channel.  Else top = floorf(in_y), bot = ceilf(in_y), ly = in_y - top, likewise left, right, lx;
 *     t = tl + (tr - tl) * lx; b = bl + (br - bl) * lx; out = t + (b - t) * ly.  A flipped box (y1 > y2) samples flipped.
 *   Output: d_out [batch n][C][pool_h][pool_w] (layout 0) or [batch n][pool_h][pool_w][C] (layout 1), rows in the order of the boxes; d_levels [batch n] int32 (may
 *     be NULL), 2 .. 5.
 *   How: one launch, a block per box and 4096 outputs; the level, and per output row / column the two texels and the weight, are computed once into LDS, not per
 *     channel.  Layout 1: the lanes run along C, with 16-byte loads and stores when C % 4 == 0 and the four maps and d_out are 16-byte aligned, scalar otherwise.
 *     Layout 0: consecutive lanes take consecutive output columns of a channel plane.
 *   IFX_E_INVALID: a NULL pointer other than d_levels, an unknown layout, batch, channels, n or an image or map size < 1, pool_h or pool_w outside 1 .. 128, a map
 *     above 2^31 - 1 texels, more than 2^30 outputs per box or more than 2^31 - 1 blocks.
 * ifx_keras_detections, one image: d_rois [R][4] normalised, d_probs [R][C], d_deltas [R][C][4]; window (y1, x1, y2, x2) in pixels, on the host.
 *   1 class = the first maximum of the row: best = 0; for j = 1 .. C - 1: probs[j] > probs[best] -> best = j (a NaN never compares greater).  score =
 *   probs[class].  2 d = deltas[class] * std_dev; box = DECODE(roi, d); times image_h (y) and image_w (x); CLIP to the window; rintf (half to even) to int32, kept
 *   as floats.  3 A row is dropped if a clipped coordinate is a NaN, or if its class is 0; and, unless min_confidence == 0 (`if config.DETECTION_MIN_CONFIDENCE:`),
 *   if not score >= min_confidence (a NaN score fails).  With min_confidence == 0 a NaN score stays and is ordered last.  4 Per class, TFNMS(the class's boxes by
 *   descending score, then ascending row; nms_threshold; max_instances).  Integer boxes of zero area neither suppress nor are suppressed.  5 Of all kept rows the
 *   max_instances best by descending score, then ascending row.
 *   Output: d_detections [max_instances][6], rows y1, x1, y2, x2, class, score as floats, zero rows behind them; d_boxes_norm [max_instances][4] (may be NULL),
 *   those boxes divided by image_h (y) and image_w (x) -- what the mask branch's ifx_pyramid_roi_align takes (model.py:1961-1963); d_index [max_instances] int64
 *   (may be NULL), each detection's ROI row, -1 behind them; d_count one int32.  The rows are what ifx_unmold_detections takes.
 *   How: a wave per row for steps 1 to 3; one block sorts all rows by (score, row); the pair mask in its TF form with the class as the group does step 4's
 *   suppression in one pass; the walk stops at max_instances kept rows -- in descending score a row with max_instances kept rows of its own class in front of it
 *   lies behind step 5's cut, so the first max_instances kept rows ARE steps 4 and 5.  Four launches.
 *   IFX_E_INVALID: R outside 1 .. 8192, C outside 2 .. 1024, max_instances outside 1 .. 8192, image_h or image_w < 1, a window coordinate that is NaN or beyond
 *   +-2^24, a NULL pointer other than d_boxes_norm and d_index. */
typedef struct ifx_keras_proposal_params { int32_t pre_nms_limit, proposal_count; float nms_threshold; float std_dev[4]; int32_t image_h, image_w; } ifx_keras_proposal_params;
typedef struct ifx_keras_detection_params {
    float std_dev[4]; float min_confidence, nms_threshold; int32_t max_instances, image_h, image_w; float window[4];
} ifx_keras_detection_params;
int ifx_keras_proposals(ifx_t* h, const float* d_rpn_probs, const float* d_rpn_bbox, const float* d_anchors, int n, const ifx_keras_proposal_params* p,
                        float* d_proposals, int64_t* d_index, int32_t* d_count, void* stream);
int ifx_pyramid_level_thresholds(int image_h, int image_w, float* out3);
int ifx_pyramid_roi_align(ifx_t* h, const float* const* d_features, const int32_t* heights, const int32_t* widths, int batch, int channels, int layout,
                          const float* d_boxes, int n, int image_h, int image_w, int pool_h, int pool_w, float* d_out, int32_t* d_levels, void* stream);
int ifx_keras_detections(ifx_t* h, const float* d_rois, const float* d_probs, const float* d_deltas, int R, int C, const ifx_keras_detection_params* p,
                         float* d_detections, float* d_boxes_norm, int64_t* d_index, int32_t* d_count, void* stream);
/* ---- the three device forms on a spatially sharded map: a deployment has ONE detector, on one rank's GPU (no counterpart in the reference: one GPU, host masks).
 * ifx_owner_segmentation_begin_device / _rois / _detections join the state machine of ifx_owner_segmentation_begin: 1 = an exchange point is pending (reduce what
 * ifx_owner_exchange(h, 200, ...) lists, then ifx_owner_segmentation_resume), 0 = complete.  ifx_owner_process_segmentation_device / _rois / _detections are the
 * same in one call each, the exchanges done on the handle's communicator (flags bit 0 then runs ifx_owner_knn_vote_colour, as ifx_owner_process_segmentation does).
 *   rgb, depth     host pointers for the superpixel refinement (flags bit 1), exactly as ifx_owner_segmentation_begin takes them; read before the begin form returns.
 *   tensors        as the unsharded entry of the same name documents them: formats, the threshold rule, the ROI paste, roi_size 1 .. 64, the mask head's stage.
 *   root = -1      every rank holds the tensors and ingests its own copy; no record, no extra exchange point; n == 0 returns 0 at once.
 *   root = r       (0 <= r < n_ranks; 0 for n_ranks = -1) only rank r's tensor pointers, n, d_count, R, C, p and stream are read; the other ranks may pass NULL / 0.
 *                  max_n (1 .. 256), roi_size / M, the form, threshold (ROI and detections forms: every rank applies its own to the record's ROI masks) and the
 *                  flags must be equal on all ranks.  max_n is the record's capacity: n > max_n on rank r is IFX_E_INVALID.
 * With root = r the call's FIRST exchange point is the record: ifx_owner_exchange(h, 200, ...) lists exactly one buffer, the record, with its size in bytes (a
 * multiple of 4, a function of form, max_n, M and the frame size only) and op 4 | r << 8 (broadcast from rank r).  Rank r wrote it on its main stream behind an
 * event recorded on `stream`: no host synchronisation.  The first resume reads the header (one 32-byte copy), checks it against this rank's arguments -- a wrong
 * magic, form, M, P or max_n means the ranks disagree: IFX_E_STATE, the call is over --, ingests from the record on every rank, rank r included (identical kernels
 * on identical bytes), and goes on into the exchange points of the host form (option own_lazy_ids' keys, the boxes, ...).  n == 0 in the header ends the call with
 * 0 on every rank after that one exchange.  The record is one allocation per handle, grown on demand: a repeated call of the same sizes allocates nothing.
 * The record, int32 words (P = width x height):
 *   header[8]   magic 0x49465852, form (1 image bits, 2 ROI masks), n, M (form 1: 0), P, max_n, 0, 0
 *   cls[max_n]  the caller's class ids in the caller's order (detections form: of the kept rows, after d_class_map); rows >= n are zero
 *   form 2      boxes f32[max_n][4], rois f32[max_n][M][M]; rows >= n are zero
 *   form 1      bits u32[max_n][ceil(P / 32)]: bit b of word j of mask m = pixel 32 j + b of mask m, binarised by the bridge's rule (u8 / bool: non-zero;
 *               f32: > threshold, a NaN is outside); bits past P and rows >= n are zero
 * The ingest from bits (popcount areas, the bridge's stable order, the gather with the overlap clean) leaves byte for byte the masks and sorted class ids that
 * ifx_process_segmentation_device's ingestion makes of the same tensors; form 2 runs the ROI entry's ingestion on pointers into the record.
 * Detections form: the mask head's stage runs on the reading rank(s) only; *out_kept is written there.  More kept rows than max_n: IFX_E_CAPACITY -- from the begin
 * form with root = -1; with root = r the record carries the count and no rows, so that EVERY rank's first resume returns IFX_E_CAPACITY and the call is over everywhere.
 * Refusals (nothing enqueued, the handle stays usable, ifx_last_error starts with the entry's name): IFX_E_STATE for a handle not created for a sharded map and for
 * a call already in flight; IFX_E_INVALID for flags bit 0 on a begin form, root outside -1 .. n_ranks - 1, max_n outside 1 .. 256, roi_size / M outside 1 .. 64
 * (every rank), n > max_n and whatever the unsharded entry of the form refuses in its arguments (the reading rank).  A refusal on rank r alone leaves the other
 * ranks waiting at the record's exchange point, and a header mismatch ends the call only on the ranks that see it (rank r's own header always matches): a rank
 * whose peers' call is over ends its own with ifx_owner_segmentation_abort (any form of the call, the host form too; 0 when nothing is in flight; the next call's
 * label scan then covers every surfel). */
int ifx_owner_segmentation_abort(ifx_t* h);
int ifx_owner_segmentation_begin_device(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const void* d_masks, int mask_format, float threshold,
                                        const int32_t* d_class_ids, int n, int frame, int flags, void* stream);
int ifx_owner_segmentation_begin_rois(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const float* d_roi_masks, int roi_size, const float* d_boxes,
                                      float threshold, const int32_t* d_class_ids, int n, int frame, int flags, void* stream);
int ifx_owner_segmentation_begin_detections(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const float* d_mask_logits, const float* d_boxes,
                                            const float* d_scores, const int64_t* d_labels, const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M,
                                            const ifx_mask_head_params* p, float threshold, int frame, int flags, void* stream, int32_t* out_kept);
int ifx_owner_process_segmentation_device(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const void* d_masks, int mask_format, float threshold,
                                          const int32_t* d_class_ids, int n, int frame, int flags, void* stream);
int ifx_owner_process_segmentation_rois(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const float* d_roi_masks, int roi_size, const float* d_boxes,
                                        float threshold, const int32_t* d_class_ids, int n, int frame, int flags, void* stream);
int ifx_owner_process_segmentation_detections(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const float* d_mask_logits, const float* d_boxes,
                                              const float* d_scores, const int64_t* d_labels, const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M,
                                              const ifx_mask_head_params* p, float threshold, int frame, int flags, void* stream, int32_t* out_kept);
/* Deferred segmentation on a spatially sharded map: a slow detector's masks of frame t, applied at frame t + k to the map as it is then (the unsharded pair is
 * ifx_segmentation_snapshot / ifx_process_segmentation_deferred*, which keep refusing a sharded handle).  Every rank makes the same calls behind the same frames.
 *
 * ifx_owner_segmentation_snapshot(h, flags): enqueue-only on the handle's stream.  Pins the whole replicated id image as creation numbers, the pose block, with
 * flags bit 1 the raw rgb / depth of the frame just processed, and per pixel THIS rank's slot of the surfel as a hint (one bisection, here and in no later launch) or
 * "another rank's".  Returns the ticket: tickets come from the handle's one counter, so ranks that make the same calls hold the same numbers.  The ticket table,
 * option seg_snapshots, the generation that ifx_map_upload bumps, ifx_segmentation_snapshot_release and _stats are the unsharded tickets' own; on a sharded ticket
 * _stats reports `pixels` of the whole image (equal on every rank) and `lost` = the pixels whose surfel THIS rank owned and lost (the ranks' sum is the unsharded
 * figure).  Under option own_lazy_ids the image is completed first: in place and collectively with the library's communicator; with a caller-driven transport the
 * call returns IFX_E_STATE and names ifx_owner_ids_begin.
 *
 * ifx_owner_segmentation_begin_deferred (host masks, sorted as for ifx_owner_segmentation_begin) and ifx_owner_segmentation_begin_deferred_device (image masks on
 * rank root's GPU, or on every rank's with root = -1; arguments as ifx_owner_segmentation_begin_device without rgb / depth: the superpixels are cut from the
 * ticket's frame, read in place on the device) return 1 / 0 like the ordinary begin forms and go on through ifx_owner_segmentation_resume and
 * ifx_owner_exchange(h, 200, ...): the record (root >= 0), the boxes, the model depth, the eviction statistics, the boxes again -- never the id image's keys.
 * ifx_owner_process_segmentation_deferred[_device] are the one-call forms on the library's communicator (flags bit 0 there: the kNN smoothing after the call).
 * Per rank the semantics are the unsharded deferred call's: a pixel keeps its surfel on the owning rank if the surfel is still stored, alive, and not today's
 * "surfel 0" -- the lowest live creation number of any rank, the word the last frame's id resolve used (creation number 0 under own_first_live = 0); every other
 * pixel reads "no surfel of this rank".  The camera centre of the model depth is the ticket's pose.  A call that completes releases its ticket on every rank; so
 * do n == 0 and a call on an empty shard.  With no frame between snapshot and call the result is the ordinary sharded call's bit for bit; at any lag it is the
 * unsharded deferred call's (maps merged by creation number).
 *
 * Refusals (nothing enqueued, the handle stays usable, ifx_last_error starts with the entry's name): IFX_E_STATE for an unsharded handle, more than one camera
 * context, a segmentation call in flight, no frame processed yet, a ticket older than an ifx_map_upload, flags bit 1 on a ticket taken without its frame;
 * IFX_E_INVALID for an unknown or released ticket, flags bit 0 on a begin form, and whatever the ordinary form refuses in its arguments; IFX_E_CAPACITY for one
 * ticket more than seg_snapshots allows.  A refused or failed call keeps its ticket.
 * Not offered (yet): the ROI, detections and unmolded forms of the deferred call, and camera contexts. */
int ifx_owner_segmentation_snapshot(ifx_t* h, int flags);
int ifx_owner_segmentation_begin_deferred(ifx_t* h, int ticket, const uint8_t* masks, const int32_t* class_ids, int nm, int frame, int flags);
int ifx_owner_segmentation_begin_deferred_device(ifx_t* h, int ticket, int root, int max_n, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids,
                                                 int n, int frame, int flags, void* stream);
int ifx_owner_process_segmentation_deferred(ifx_t* h, int ticket, const uint8_t* masks, const int32_t* class_ids, int nm, int frame, int flags);
int ifx_owner_process_segmentation_deferred_device(ifx_t* h, int ticket, int root, int max_n, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids,
                                                   int n, int frame, int flags, void* stream);
/* bestIDInEachSurfel (IF/Core/InstanceFusionCuda.cu:1158-1200) for the live surfels, map order. */
int ifx_labels(ifx_t* h, int32_t* out, int max_n);
/* InstanceFusion::renderProjectMap (IF/Core/InstanceFusion.cpp:1232-1252, renderProjectFrameKernel IF/Core/InstanceFusionCuda.cu:1432-1498): the
 * instance colour of the surfel under every pixel of the id image after fusion -- what getProjectColorMap_gpu() hands to the GUI: H x W x 4
 * floats (r, g, b in [0,1], alpha 1; black where no stable surfel is visible).  out_rgba: host buffer or NULL; d_out_rgba: device buffer or NULL
 * (enqueue only, no synchronisation).  The 2-D boxes the reference draws on top on the host are not drawn. */
int ifx_render_project_map(ifx_t* h, float* out_rgba, float* d_out_rgba);
/* Free-viewpoint render of the map: the surfel pass of the reference's main window -- GlobalModel::renderPointCloud (draw_global_surface.vert / .geom / .frag,
 * EF/GlobalModel.cpp:328-391) and GlobalModel::renderGlobalID (draw_global_ID.*) -- from any camera on a viewport of any size.
 *   mvp          4 x 4, row-major: clip = mvp . (x, y, z, 1) of a world point.  The reference's camera is Pangolin's ProjectionMatrix(w, h, fu, fv, u0, v0, zNear, zFar) times
 *                the inverse pose (viewer_mvp in the Python package, ifx::viewerMvp in ifx_host.hpp): clip.x = (2 fx / w) X + (1 - 2 cx / w) Z,
 *                clip.y = -(2 fy / h) Y - (1 - 2 cy / h) Z, clip.z = (far + near) / (far - near) Z - 2 far near / (far - near), clip.w = Z in the camera frame (y down,
 *                z forward).  With the frame's intrinsics at the tracked pose the output has the orientation of pred_image.
 *   w, h         the viewport, 1..4096 each, unrelated to the frame's size.
 *   threshold    a surfel is drawn if its confidence is above it, or if `unstable`; NaN: the handle's confidence threshold.  A surfel at or below it is pushed back
 *                by its radius in depth (draw_global_surface.frag:35-42).  A surfel whose instance-colour word is -1 is never drawn (.vert:44).
 *   color_type   0 shaded grey, 1 normal, 2 the colour word, 3 a ramp of the creation time against `time`, 4 the instance-colour word; then dimmed by 0.25 when
 *                draw_window and time - lastUpdate > time_delta, then blended 0.6 / 0.4 with the shaded grey (.geom:50-88).
 *   time         < 0: the handle's tick.  time_delta < 0: the handle's.  clear_rgb: the colour where nothing is drawn (the GUI clears to white).
 * Outputs, top row first (output row r is GL window row h - 1 - r), host (out_*), device (d_out_*), both or neither of each:
 *   rgba  h x w x 4 floats: the base colour of the nearest surfel (per surfel, not interpolated), alpha 1; clear_rgb with alpha 0 where nothing was drawn
 *   ids   h x w int32: the slot of that surfel in the numbering of ids_after; -1 where nothing was drawn (there is no "surfel 0" rule here)
 * Rasterised as GL does it (quads of four separately projected corners, 1/256 px snap, top-left rule, perspective-correct texcoord, 24-bit depth cleared to 1 with
 * GL_LESS, ties to the lower slot), with ONE deviation: a quad with a corner at clip.w <= 0 or more than 65536 px outside the window is not drawn, where GL clips
 * it and draws the visible part.  Read-only on the map; enqueued on the main stream behind the last frame; the host is synchronised only
 * when a host output is given.  IFX_E_INVALID: w or h outside 1..4096, color_type outside 0..4, a non-finite mvp (nothing is written).  IFX_E_STATE: a sharded
 * handle, or between the stage calls of a frame.
 * ifx_render_view_big_quads: how many quads of the last call covered more than 256 pixels and were drawn by a workgroup each (synchronises the main stream). */
typedef struct { float mvp[16]; int32_t w, h; float threshold; int32_t color_type, unstable, draw_window, time, time_delta; float clear_rgb[3]; } ifx_view_params;
int ifx_render_view(ifx_t* h, const ifx_view_params* p, float* out_rgba, int32_t* out_ids, float* d_out_rgba, int32_t* d_out_ids);
int ifx_render_view_big_quads(ifx_t* h);
/* The same render of a spatially sharded map (ifx_config::n_ranks), where no rank holds the whole map.  RULE: the rule of ifx_render_view with one change -- the low
 * word of a pixel's key is the surfel's CREATION NUMBER, not its slot.  Creation numbers are the same on every rank and ascend with the slots of the unsharded,
 * compacted map, so a depth tie goes to the lower creation number on every rank, which is ifx_render_view's "lower slot": rgba equals the unsharded render of the
 * merged map bit for bit, and ids holds creation numbers (the slots of that map through ifx_map_seq's numbering), -1 where nothing is drawn (creation numbers stop at
 * 0xFFF00000).  Every rank makes the calls with the same parameters and gets the whole image.
 *   ifx_owner_render_view_begin(h, p, want_rgba, want_ids)   draws this rank's shard into the viewer's key image.  Returns 1: an exchange is pending, 0: nothing was
 *       asked for (neither output wanted), < 0: refused.
 *   ifx_owner_render_view_resume(h, out_rgba, out_ids, d_out_rgba, d_out_ids)   continues behind the exchange; 1: another exchange is pending (the outputs are not
 *       yet read or written), 0: the outputs are written (host, device, both or neither of each wanted image, as ifx_render_view).  An output begin was not
 *       asked for is IFX_E_INVALID.
 *   The pending exchange is listed by ifx_owner_exchange under 400 -- the key image, op 0 (u64 MIN), 8 B / pixel -- and then, only when rgba is wanted, under 401 --
 *       the colour block, in which the owner of each pixel's winner has written the colour and every other rank zeros, op 1 (i32 SUM), 16 B / pixel.  An ids-only
 *       call has one exchange.
 *   ifx_owner_render_view   the same as ONE call when the library holds the communicator (ifx_owner_init_comm / ifx_owner_set_comm): its collectives are counted by
 *       ifx_owner_exchange_stats (1 and 8 B / pixel, or 2 and 24 B / pixel with rgba); enqueue only unless a host output is given.
 *   ifx_owner_render_view_big_quads   the big-quad count of THIS rank's shard in the last call.
 * IFX_E_INVALID exactly where ifx_render_view returns it.  IFX_E_STATE: an unsharded handle; between the phases of a frame (ifx_owner_frame_phase) or of a predict;
 * while a segmentation call or an id render waits for its exchange; _begin while a render is pending, _resume without _begin; ifx_owner_render_view without a
 * communicator.  Nothing is written by a refused call.  Read-only on the map: only the viewer's own buffers are written or exchanged, and the key image is all-empty
 * again when the call ends.  ifx_render_view itself keeps refusing sharded handles. */
int ifx_owner_render_view_begin(ifx_t* h, const ifx_view_params* p, int want_rgba, int want_ids);
int ifx_owner_render_view_resume(ifx_t* h, float* out_rgba, int32_t* out_ids, float* d_out_rgba, int32_t* d_out_ids);
int ifx_owner_render_view(ifx_t* h, const ifx_view_params* p, float* out_rgba, int32_t* out_ids, float* d_out_rgba, int32_t* d_out_ids);
int ifx_owner_render_view_big_quads(ifx_t* h);
/* ---- instance ground truth (the reference's ScanNet evaluation).
 * ifx_set_instance_gt: the instanceGT argument of ElasticFusion::processFrame (EF/ElasticFusion.h:79, EF/ElasticFusion.cpp:285-291): H x W bytes; surfels created by the
 *   frames that follow remember the id under the pixel that created them (vImgCorr.w, data.vert:215-228; -2 without ground truth).  NULL switches it off.
 * ifx_precision_recall: computePrecisionAndRecallKernel (IF/Core/InstanceFusionCuda.cu:2085-2114), the device half of InstanceFusion::evaluateAndSave
 *   (IF/Core/InstanceTable.cpp:336-370): surfels per instance (by instance colour), per ground-truth id, and per (ground-truth id, instance) pair. */
int ifx_set_instance_gt(ifx_t* h, const uint8_t* gt_hw);
int ifx_precision_recall(ifx_t* h, int32_t* inst_num96, int32_t* gt_num256, int32_t* inst_gt_map_256x96);
/* class id per instance slot, -1 = unused (getInstanceTable, IF/Core/InstanceFusion.h:87) */
int ifx_instance_table(ifx_t* h, int32_t* out96);
/* getLoopClosureInstanceTable, IF/Core/InstanceTable.cpp:98-121: int[96*5] = r,g,b,class,index */
int ifx_loop_closure_instance_table(ifx_t* h, int32_t* out480);
/* ---- duplicate instances after a loop closure (what the reference wrote and switched off: InstanceFusion::checkLoopClosure, IF/Core/InstanceTable.cpp:122-169, its
 * call commented out at IF/main.cpp:143; loopClosureCopyMatchInstanceKernel, IF/Core/InstanceFusionCuda.cu:1370-1427; cleanInstanceTable / cleanInstanceTableMap).
 * ifx_merge_instances: pairs = n entries (from, to), 0 <= n <= 95.  For every surfel slot below the count (tombstones included) and every pair, in ascending `from`:
 *   f = the from-counter as decoded; if f > 0 the target's word is decoded, f added to the target's half, clamped (>= 65535 -> 65535), encoded and stored; if f <= 0
 *   the target's word stays bit for bit (the -1 of a first-frame surfel is "not projected", not a count: the reference would make it -2).  Then every from-half is
 *   cleared as a table eviction clears it, inst_class[from] = -1, the full label scan runs, and a live surfel that carries the table colour of a cleared slot takes
 *   the colour of its new label (the default colour 7434609 for label -1).  Returns with the stream drained.  One pass over the vote store; a record of which no
 *   word changed is not written.
 *   IFX_E_INVALID, nothing enqueued and nothing changed: an id outside 0 .. 95, from == to, a from or to whose slot is unused, a from named twice, or a chain (an
 *   id that is the target of one pair and the source of another: the reference's loop would lose the far end's votes -- resolve chains to their roots first, as
 *   the wrappers do).  n == 0: IFX_OK, nothing done.  A deferred-segmentation ticket taken before the call stays valid.
 *   Sharded handles (n_ranks > 1, ifx_set_shard): every rank makes the same call with THE SAME pairs on its shard; the table is replicated, nothing is exchanged.
 * ifx_instance_duplicates: over the current id image (completed if lazy) the projected box of every instance, as the segmentation call computes them.  Registered
 *   instances l < h of one class are duplicates when both boxes are non-empty and I / U > iou_thresh in the float arithmetic of computeCompareMap
 *   (IF/Core/InstanceFusion.cpp:595-651) with the second box in the mask's place; instance 0 may be a target.  Every h takes its best l (largest I / U, ties to the
 *   lower index), chains are resolved to their roots, and out_pairs receives (from = h, to = root) ascending in from: ready for ifx_merge_instances.  Returns the
 *   number of pairs found (at most max_pairs are written; 95 always suffice).  Changes no state.  IFX_E_STATE on a sharded handle. */
int ifx_merge_instances(ifx_t* h, const int32_t* pairs, int n);
int ifx_instance_duplicates(ifx_t* h, float iou_thresh, int32_t* out_pairs, int max_pairs);
int ifx_mask_clean_overlap(ifx_t* h, uint8_t* masks, int n);  /* IF/Core/InstanceFusionCuda.cu:118-141 (host in/out) */
/* maskGeometricFilter + filterAreaCompute (IF/Core/InstanceFusion.cpp:470-593) as a stage, host buffers: depth = model
 * depth under the camera (u16 H x W, 1186 units per metre, what getProjectDepthMap :977-996 produces); masks n x H x W
 * in/out; ori = the masks before clean-overlap; unavailable n bytes in/out (set entries are skipped). */
int ifx_mask_geometric_filter(ifx_t* h, const uint16_t* depth, uint8_t* masks, const uint8_t* ori, int n, uint8_t* unavailable);
/* The mask rule of the compare map as a stage (the reference's compareMapType 2: getProjectInstanceListKernel, IF/Core/InstanceFusionCuda.cu:781-807,
 * maskCompareMapKernel :826-881, the decision loop IF/Core/InstanceFusion.cpp:834-861), whatever option "compare_map" says.  masks: host, n x H x W, used as
 * given (> 0 is inside); class_ids n; unavailable n bytes or NULL.  Reads the current id image (completed if lazy), the current votes and the instance table;
 * changes no state.
 *   presence(i, p): the id image names a surfel of this map under pixel p and counter i of that surfel decodes to > 0.  Md(m, p) / Id(i, p): some pixel of p's
 *   3 x 3 neighbourhood inside the image has mask m > 0 / presence(i, .).  I[m][i] = #{p : Md and Id}, U[m][i] = #{p : Md or Id} = A_M[m] + A_I[i] - I[m][i]
 *   over all pixels; pairs whose classes differ (every unused slot, class -1, included) stay 0.
 *   decision per mask: none if it is unavailable or its box over the pixels that carry a surfel is degenerate (the box rule's test); otherwise over the instances
 *   of its class in ascending order, iou = float(I) / float(U), a candidate iff iou > 0.5f, the best replaced iff iou > the best so far (equal maxima keep the
 *   lowest index; 0 / 0 matches nothing); and a best of instance 0 is NO match, as under the box rule.
 * out_I, out_U: n x 96 or NULL; out_best: n (the matched instance or -1) or NULL.  IFX_E_INVALID: n outside 0..256, NULL masks or class ids with n > 0;
 * IFX_E_STATE: a sharded handle. */
int ifx_mask_compare_map(ifx_t* h, const uint8_t* masks, const int32_t* class_ids, int n, const uint8_t* unavailable, int32_t* out_I, int32_t* out_U, int32_t* out_best);
/* What the last segmentation call on this handle decided per mask (the reference prints it, IF/Core/InstanceFusion.cpp:955-1010), under either rule and either
 * schedule: returns the call's mask count (0: none yet, or a call without masks or on an empty map) and fills the first min(count, max_n) entries of
 * out_best -- the compare map's match, -1 if none (after an eviction: of the map recomputed for the mask that caused it and those behind it) -- and out_target
 * -- the instance the mask voted for (its match, or the slot it registered), -1 if it was unusable.  Masks are in the call's order (device entries: sorted).
 * The owners' calls of a sharded map are not recorded. */
int ifx_segmentation_matches(ifx_t* h, int32_t* out_best, int32_t* out_target, int max_n);

/* ---- superpixel refinement stages (the three calls of processInstance steps -1_1..-1_3,
 * IF/Core/InstanceFusion.cpp:722-738; ifx_process_segmentation runs them when flags bit1 is set).
 * All buffers are host memory, images are H x W row-major.
 * ifx_slic_segment: gSLICrInterface (IF/Core/InstanceFusion_superpixel.cpp:713-772; gSLICr with
 *   spixel_size 16, coh_weight 0.6, 5 iterations, XYZ, enforce connectivity): rgb H x W x 3 u8 ->
 *   superpixel label per pixel; returns the number of superpixels (> 0) or a negative error.
 * ifx_merge_superpixels: mergeSuperPixel (IF/Core/InstanceFusion_superpixel.cpp:40-225): seg is the
 *   SLIC labelling on entry and the re-clustered labelling (-1 = no geometry) on return, final_out the
 *   merged region id per pixel, info_out (optional) the spNum x 30 float table in the reference's SPI_*
 *   layout (:12-33).  Returns spNum.
 * ifx_mask_superpixel_filter: maskSuperPixelFilter_OverSeg (:651-710): a mask keeps a merged region
 *   iff it covers more than 75 % of it; masks n x H x W u8 rewritten in place. */
/* flannKnnVoteSurfelMap + mapKnnVoteColourKernel (IF/Core/InstanceFusion.cpp:1070-1163, IF/Core/InstanceFusionCuda.cu:1237-1340)
 * as a stage: every live surfel takes the colour of the instance most of its 10 nearest surfels (itself included) are
 * labelled with, using the labels of the last segmentation call.  nbr_out (optional, [max_n][10] int32, host) receives
 * the neighbour slots of the first max_n slots, -1 = none. */
int ifx_knn_vote_colour(ifx_t* h, int32_t* nbr_out, int max_n);
int ifx_slic_segment(ifx_t* h, const uint8_t* rgb, int32_t* seg_out);
int ifx_merge_superpixels(ifx_t* h, const uint16_t* depth, int32_t* seg_inout, int32_t* final_out, float* info_out);
int ifx_mask_superpixel_filter(ifx_t* h, const int32_t* final_ids, uint8_t* masks, int n);

/* ---- measurement hooks */
/* Per-stage GPU time of the frames processed since the last reset, from HIP events on the handle's
 * streams: ms[0]=track, ms[1]=fuse (all map passes), ms[2]=instance, ms[3]=frame side (bilateral, frame pyramids,
 * SO(3); runs concurrently with the others when a frame is announced ahead).  Stages 0, 1, 3 are recorded only while
 * ifx_set_option(h, "stage_timing", 1) is on: every event record is a marker packet on the queue and the eight of a
 * frame cost about 4 % of the frame rate. */
int ifx_stage_ms(ifx_t* h, float* ms4, int reset);
/* Superpixels run ahead of a segmentation call.  When ifx_should_segment answers "not this frame" but its cadence says the NEXT frame will end with a call, and
 * that frame is announced (ifx_hint_next_frame_device), SLIC + the superpixel merge of the announced frame -- work that reads the frame only, about half of a call's
 * dispatches (gSLICr + IF/Core/InstanceFusion.cpp:722-738 steps -1_1, -1_2) -- are enqueued on the side stream at once, under that frame's tracker and map passes;
 * ifx_process_segmentation(rgb = depth = NULL) of that frame then waits for one event instead of running them.  Same kernels, same images, same result.
 * ms: device time of the runs on the side stream (NOT part of ifx_stage_ms's "instance", which is the main-stream span of the calls); runs / used: how many were
 * enqueued and how many a call consumed (a hint that does not come true leaves its run unused).  Option "slic_ahead" 0 turns the look-ahead off. */
int ifx_superpixel_ahead_stats(ifx_t* h, float* ms, int32_t* runs, int32_t* used, int reset);
/* The one-frame look-ahead in numbers (diagnostics, tests; no counterpart in the reference): out3 = frames of this handle (unsharded entries) that found their frame
 * side already computed (ifx_prefetch_ / ifx_hint_next_frame*), frames whose tracker had run ahead, frames that came through ifx_hint_next_frame (host pointers). */
int ifx_lookahead_stats(ifx_t* h, int32_t* out3, int reset);
/* Average duration (ms) of the named kernel over its launches since the last reset, measured with
 * HIP events around each launch (enabled by ifx_set_option("kernel_timing",1)). */
int ifx_kernel_ms(ifx_t* h, const char* kernel, float* avg_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* IFX_C_API_H_ */
