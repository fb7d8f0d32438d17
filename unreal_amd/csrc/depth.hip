// Depth prediction for first-person mazes, for gfx950: the labels and the loss.
//
// unreal_maze_depth_labels: the depth class of 12 frame columns of every actor's current view, from the actor's cell,
// heading and walls alone.  Position j is frame column i = 7 j + 3, the centre of a 7-column band; its ray is the DDA of
// maze.hip's fp_render restated (camera: maze.hip's header comment; every quantity a ratio of small integers), which gives
// t = tn / td at the first wall cell or map border.  The class is the number of edges e in {1, 2, 3, 4, 6, 8, 12} with
// t >= e, decided as tn >= e td in integers: a ray that ends exactly on an edge (q = 21: t = 2 (2m + 1)) is in the upper
// class.  Pickups, the goal and wall styles do not change it.  16 lanes per actor (12 cast a ray), 16 actors per
// workgroup; the wall bits are read from the block's layout record or the actor's own (a generated maze) through the
// cache: nothing is staged in LDS.
//
// unreal_depth_loss_grad: softmax cross-entropy of the head's 12 groups of 8 logits against those labels, its gradient
// and the hit count, one thread per (row, position).
#include "common.h"
#include "maze_common.h"

namespace {

constexpr int kDepthPositions = 12, kDepthClasses = 8;      // UNREAL_DEPTH_POSITIONS / UNREAL_DEPTH_CLASSES
constexpr int kLanesPerActor = 16, kActorsPerGroup = 256 / kLanesPerActor;
static_assert(7 * (kDepthPositions - 1) + 3 < FRAME_W && kDepthPositions <= kLanesPerActor, "depth columns");

// `heading`: heading[B] (record_words 0) or the B per-actor records of record_words int32 whose word 0 is the heading.
// `layout` null: a generated block, whose actors' wall bits begin at word kNavActorWords of their record.
__global__ __launch_bounds__(256) void maze_depth_labels_kernel(int B, int H1, int N, const int* __restrict__ count,
                                                                const int* __restrict__ pos,
                                                                const int* __restrict__ heading, int record_words,
                                                                const int* __restrict__ cfg,
                                                                const int* __restrict__ layout,
                                                                uint8_t* __restrict__ r_depth) {
  // (uniform) as the step kernels: a block of another grid size, or of the other kind, writes nothing
  if (cfg[0] != N || ((cfg[2] & kMazeGen) != 0) != (layout == nullptr)) return;
  const int b = blockIdx.x * kActorsPerGroup + threadIdx.x / kLanesPerActor, j = threadIdx.x % kLanesPerActor;
  if (b >= B || j >= kDepthPositions) return;
  const int stride = record_words ? record_words : 1;
  const int* rec = layout ? maze_rec(cfg, maze_layout(cfg, layout, b)) : heading + (size_t)b * stride + kNavActorWords;
  const int ex = pos[2 * b], ey = pos[2 * b + 1], h = heading[(size_t)b * stride] & 3;
  const int dx = (h == 0) - (h == 2), dy = (h == 1) - (h == 3);
  const int rx = -dy, ry = dx;
  const int i = 7 * j + 3, q = 2 * i + 1 - FRAME_W, aq = abs(q), sg = q > 0 ? 1 : -1;
  int f = 0, sd = 0, k = 0, m = 0, tn = 1, td = 2;
  for (int it = 0; it < 2 * N + 2; ++it) {        // at most 2N cells before the ray leaves the map
    if ((2 * k + 1) * aq < (2 * m + 1) * FRAME_W) {
      ++f; tn = 2 * k + 1; td = 2; ++k;
    } else {
      sd += sg; tn = (2 * m + 1) * FRAME_W; td = 2 * aq; ++m;
    }
    const int cx = ex + f * dx + sd * rx, cy = ey + f * dy + sd * ry;
    if (cx < 0 || cx >= N || cy < 0 || cy >= N) break;
    const int c = cy * N + cx;                     // < 441: inside the record's 14 wall words
    if (((uint32_t)rec[c >> 5] >> (c & 31)) & 1u) break;
  }
  const int cls = (tn >= td) + (tn >= 2 * td) + (tn >= 3 * td) + (tn >= 4 * td) + (tn >= 6 * td) + (tn >= 8 * td) +
                  (tn >= 12 * td);
  const int slot = count[b] % H1;
  r_depth[((size_t)b * H1 + slot) * kDepthPositions + j] = (uint8_t)cls;
}

__global__ __launch_bounds__(256) void depth_loss_grad_kernel(int rows, const float* __restrict__ logits, int ld,
                                                              const uint8_t* __restrict__ r_depth,
                                                              const int* __restrict__ frame_idx,
                                                              const int* __restrict__ active, float scale,
                                                              float* __restrict__ dlogits, float* __restrict__ loss,
                                                              int* __restrict__ hits) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int r = g / kDepthPositions, j = g - r * kDepthPositions;
  float l = 0.f;
  int hit = 0, counted = 0;
  if (r < rows) {
    const bool on = active[r] != 0;
    float* d = dlogits ? dlogits + (size_t)r * (kDepthPositions * kDepthClasses) + j * kDepthClasses : nullptr;
    if (on) {
      const float* z = logits + (size_t)r * ld + j * kDepthClasses;
      const int label = min((int)r_depth[(size_t)frame_idx[r] * kDepthPositions + j], kDepthClasses - 1);
      float v[kDepthClasses];
#pragma unroll
      for (int c = 0; c < kDepthClasses; ++c) v[c] = z[c];
      float mx = v[0], zl = v[0];
      int arg = 0;
#pragma unroll
      for (int c = 1; c < kDepthClasses; ++c) {
        if (v[c] > mx) { mx = v[c]; arg = c; }     // the lowest index on ties
        zl = c == label ? v[c] : zl;               // (selects: a dynamically indexed register array is placed in scratch)
      }
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < kDepthClasses; ++c) {
        v[c] = expf(v[c] - mx);
        s += v[c];
      }
      l = logf(s) - (zl - mx);                     // -log p[label]
      const float inv = 1.f / s;
      if (d) {
#pragma unroll
        for (int c = 0; c < kDepthClasses; ++c) d[c] = scale * (v[c] * inv - (c == label ? 1.f : 0.f));
      }
      hit = arg == label;
      counted = 1;
    } else if (d) {
#pragma unroll
      for (int c = 0; c < kDepthClasses; ++c) d[c] = 0.f;
    }
  }
  // one atomic per workgroup and sum: the waves' partial sums meet in LDS first
  __shared__ float s_l[4];
  __shared__ int s_hit[4], s_cnt[4];
  l = wave_sum(l);
  const int nh = __popcll(__ballot(hit)), nc = __popcll(__ballot(counted));
  if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = l; s_hit[threadIdx.x >> 6] = nh; s_cnt[threadIdx.x >> 6] = nc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (c) {
      atomicAdd(loss, scale * (((s_l[0] + s_l[1]) + s_l[2]) + s_l[3]));
      atomicAdd(hits, s_hit[0] + s_hit[1] + s_hit[2] + s_hit[3]);
      atomicAdd(hits + 1, c);
    }
  }
}

}  // namespace

extern "C" {

int unreal_maze_depth_labels(int B, int H1, int N, const int* count, const int* pos, const int* heading, int record_words,
                             const int* cfg, const int* layout, uint8_t* r_depth, void* stream) {
  if (B <= 0 || H1 <= 0 || !count || !pos || !heading || !cfg || !r_depth) return UNREAL_EINVAL;
  if (!(N == 7 || N == 12 || N == 14 || N == 21)) return UNREAL_EINVAL;
  if (record_words < 0 || (record_words > 0 && record_words < kNavActorWords)) return UNREAL_EINVAL;
  // a generated block's walls are in the actor's record: it must hold them
  if (!layout && record_words < gen_actor_words(N)) return UNREAL_EINVAL;
  hipLaunchKernelGGL(maze_depth_labels_kernel, dim3((B + kActorsPerGroup - 1) / kActorsPerGroup), dim3(256), 0,
                     (hipStream_t)stream, B, H1, N, count, pos, heading, record_words, cfg, layout, r_depth);
  return unreal_launch_status();
}

int unreal_depth_loss_grad(int rows, const float* logits, int ld, const uint8_t* r_depth, const int* frame_idx,
                           const int* active, float scale, float* dlogits, float* loss, int* hits, void* stream) {
  if (rows <= 0 || ld < kDepthPositions * kDepthClasses || !logits || !r_depth || !frame_idx || !active || !loss || !hits)
    return UNREAL_EINVAL;
  if ((long)rows * kDepthPositions > 0x7fffffffL - 256) return UNREAL_EINVAL;       // (thread index in int32)
  const int n = rows * kDepthPositions;
  hipLaunchKernelGGL(depth_loss_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rows, logits, ld,
                     r_depth, frame_idx, active, scale, dlogits, loss, hits);
  return unreal_launch_status();
}

}  // extern "C"
