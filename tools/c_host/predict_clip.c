/* A host WITHOUT Python for a frame-sharded clip model: runs the container written by
 * deephar_amd.parallel.ShardedClipModel.export_clip_plan through dh_clip_create / dh_clip_forward_host of
 * include/deephar_hip.h -- frame stage, all-gather, one unpack launch, temporal head: what a C replacement of
 * ShardedClipModel.predict (deephar_amd/parallel.py; the reference runs a clip on one GPU, action.py:357-366,
 * spnet.py:219-235) looks like.  Plain C, no HIP headers:
 *     gcc -O2 -Iinclude tools/c_host/predict_clip.c -Ldeephar_amd/csrc -ldeephar_hip -Wl,-rpath,$PWD/deephar_amd/csrc -o predict_clip
 *     ./predict_clip model.dhclip frames.raw out_prefix       (frames.raw: raw float32 or uint8 [m, Tl, H, W, C], as the plan says)
 * writes out_prefix.<k>.f32 per model output and prints the clips/s of a second, timed call.
 *
 * The default build is rank 0 of a world of ONE with a NULL callback: the library reads the packed tensor where the frame
 * plan left it.  With -DDH_WITH_RCCL the callback is ncclAllGather on a communicator of one rank; that build includes
 * rccl.h (which brings the HIP headers) and links -lrccl ITSELF -- libdeephar_hip.so never does:
 *     gcc -O2 -DDH_WITH_RCCL -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tools/c_host/predict_clip.c \
 *         -Ldeephar_amd/csrc -ldeephar_hip -L/opt/rocm/lib -lrccl -lamdhip64 -Wl,-rpath,$PWD/deephar_amd/csrc -o predict_clip_rccl
 * Only a world of one has been run: this program has one process and one GPU.  A multi-rank host creates one
 * communicator per rank (ncclCommInitRank with a shared id) and passes the same callback; nothing here says anything
 * about how such a run behaves across GPUs. */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include "deephar_hip.h"

#ifdef DH_WITH_RCCL
#include <rccl/rccl.h>
static int rccl_allgather(void* ctx, const float* send, float* recv, int64_t floats_per_rank, void* stream) {
  return ncclAllGather(send, recv, (size_t)floats_per_rank, ncclFloat, *(ncclComm_t*)ctx, (hipStream_t)stream) == ncclSuccess ? 0 : 1;
}
#endif

static void* slurp(const char* path, size_t* n) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  *n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc(*n ? *n : 1);
  if (fread(p, 1, *n, f) != *n) { perror("read"); exit(2); }
  fclose(f);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s model.dhclip frames.raw out_prefix\n", argv[0]); return 2; }
  size_t nb, nx;
  void* blob = slurp(argv[1], &nb);
  void* x = slurp(argv[2], &nx);
  dh_clip_info info;
  int rc = dh_clip_inspect(blob, nb, &info);
  if (rc != DH_OK) { fprintf(stderr, "dh_clip_inspect: %s\n", dh_error_string(rc)); return 1; }
  if (info.world != 1) { fprintf(stderr, "this host is one rank; the container was written for %d\n", info.world); return 1; }
  dh_allgather_fn gather = NULL;
  void* ctx = NULL;
#ifdef DH_WITH_RCCL
  ncclComm_t comm;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess || ncclCommInitRank(&comm, 1, id, 0) != ncclSuccess) { fprintf(stderr, "rccl init failed\n"); return 1; }
  gather = rccl_allgather;
  ctx = &comm;
#endif
  dh_clip* clip = NULL;
  rc = dh_clip_create(blob, nb, 0, gather, ctx, &clip);
  if (rc != DH_OK) { fprintf(stderr, "dh_clip_create: %s\n", dh_error_string(rc)); return 1; }
  free(blob);
  const int nout = dh_clip_num_outputs(clip);
  const size_t item = (size_t)dh_clip_frame_items(clip) * (dh_clip_input_is_u8(clip) ? 1 : 4);
  const int m = (int)(nx / item);
  if (m < 1 || m > dh_clip_batch(clip) || (size_t)m * item != nx) { fprintf(stderr, "bad input size\n"); return 1; }
  float** outs = (float**)calloc((size_t)nout, sizeof(float*));
  for (int k = 0; k < nout; ++k) outs[k] = (float*)malloc((size_t)dh_clip_output_items(clip, k) * 4 * (size_t)m);
  rc = dh_clip_forward_host(clip, x, m, outs);
  if (rc != DH_OK) { fprintf(stderr, "dh_clip_forward_host: %s\n", dh_error_string(rc)); return 1; }
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  rc = dh_clip_forward_host(clip, x, m, outs);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  if (rc != DH_OK) return 1;
  for (int k = 0; k < nout; ++k) {
    char path[1024];
    snprintf(path, sizeof path, "%s.%d.f32", argv[3], k);
    FILE* f = fopen(path, "wb");
    if (!f) { perror(path); return 2; }
    fwrite(outs[k], 4, (size_t)dh_clip_output_items(clip, k) * (size_t)m, f);
    fclose(f);
  }
  const double dt = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  printf("%d clips of %d frames, %d outputs, %s, %.3f ms (%.1f clips/s incl. H2D / D2H)\n", m, info.T, nout,
         gather ? "ncclAllGather callback" : "no collective (world 1)", 1e3 * dt, m / dt);
  dh_clip_destroy(clip);
#ifdef DH_WITH_RCCL
  ncclCommDestroy(comm);
#endif
  return 0;
}
