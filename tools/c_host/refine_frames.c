/* A host WITHOUT Python that runs the box-refinement loop of the MPII evaluation (exp/common/mpii_tools.py:13-52 in the
 * reference) over FULL frames with the boxes resident on the device: a uint8 plan exported by
 * deephar_amd.Model.export_plan(path, batch, uint8=True), fed through dh_frames_* / dh_refine_frames_host of
 * include/deephar_hip.h -- the frames and the initial float boxes are uploaded once, every iteration's windows come from the
 * previous iteration's poses on the GPU.  Plain C, no HIP headers:
 *     gcc -O2 -Iinclude tools/c_host/refine_frames.c -Ldeephar_amd/csrc -ldeephar_hip -Wl,-rpath,$PWD/deephar_amd/csrc -o refine_frames
 *     ./refine_frames model.dhplan frames.u8 H W boxes.f64 OH OW outidx num_iter winsize_scale momentum out_prefix
 *   frames.u8 : raw uint8 [n, H, W, 3], n full frames of one size; sample i is frame i
 *   boxes.f64 : raw float64 [n, 4], the initial boxes (x0, y0, x1, y1); n <= the plan's batch
 *   OH OW     : the crop size the model takes (the plan file does not carry it)
 * writes out_prefix.poses.f32 (raw output `outidx` of every iteration, [num_iter, n, J, D]), out_prefix.jobs.i32
 * ([num_iter, n, 6]) and out_prefix.status.i32 ([num_iter, n]), and prints every window: "window <iteration> <sample> x0 y0 x1 y1
 * status". */
#include <stdio.h>
#include <stdlib.h>
#include "deephar_hip.h"

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

static int dump(const char* prefix, const char* what, const void* p, size_t bytes) {
  char path[1024];
  snprintf(path, sizeof path, "%s.%s", prefix, what);
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 2; }
  fwrite(p, 1, bytes, f);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 13) {
    fprintf(stderr, "usage: %s plan.dhplan frames.u8 H W boxes.f64 OH OW outidx num_iter winsize_scale momentum out_prefix\n", argv[0]);
    return 2;
  }
  const int H = atoi(argv[3]), W = atoi(argv[4]), OH = atoi(argv[6]), OW = atoi(argv[7]), outidx = atoi(argv[8]), num_iter = atoi(argv[9]);
  const double winsize_scale = atof(argv[10]), momentum = atof(argv[11]);
  size_t nb, nx, nbox;
  void* blob = slurp(argv[1], &nb);
  uint8_t* px = (uint8_t*)slurp(argv[2], &nx);
  double* boxes = (double*)slurp(argv[5], &nbox);
  if (H < 1 || W < 1 || nx == 0 || nx % ((size_t)H * (size_t)W * 3) != 0 || nbox == 0 || nbox % 32 != 0 ||
      nbox / 32 != nx / ((size_t)H * (size_t)W * 3)) {
    fprintf(stderr, "bad frame or box file size (one box per frame)\n");
    return 1;
  }
  const int n = (int)(nbox / 32);
  dh_plan* plan = NULL;
  int rc = dh_plan_create(blob, nb, &plan);
  if (rc != DH_OK) { fprintf(stderr, "dh_plan_create: %s\n", dh_error_string(rc)); return 1; }
  free(blob);
  int J = 0;
  rc = dh_refine_frames_shape(dh_plan_num_inputs(plan), dh_plan_input_is_u8(plan, 0), dh_plan_input_items(plan, 0), dh_plan_batch(plan), n,
                              OH, OW, dh_plan_num_outputs(plan), outidx, dh_plan_output_items(plan, outidx),
                              dh_plan_output_channels(plan, outidx), num_iter, &J);
  if (rc != DH_OK) {
    fprintf(stderr, "this plan cannot refine %d boxes of %d x %d crops on output %d (single uint8 image input, a pose output)\n", n, OH,
            OW, outidx);
    return 1;
  }
  dh_crop_src* table = (dh_crop_src*)calloc((size_t)n, sizeof(dh_crop_src));
  int32_t* src = (int32_t*)calloc((size_t)n, sizeof(int32_t));
  for (int i = 0; i < n; ++i) {
    table[i].ptr = px + (size_t)i * (size_t)H * (size_t)W * 3;
    table[i].pitch = 3 * (int64_t)W;
    table[i].H = H;
    table[i].W = W;
    src[i] = i;
  }
  dh_frames* frames = NULL;
  rc = dh_frames_create(table, n, &frames);
  if (rc != DH_OK) { fprintf(stderr, "dh_frames_create: %s\n", dh_error_string(rc)); return 1; }
  free(px);                                                   /* the frames live on the device now */
  free(table);
  const size_t items = (size_t)dh_plan_output_items(plan, outidx), rows = (size_t)num_iter * (size_t)n;
  float* poses = (float*)malloc(rows * items * 4);
  dh_crop_job* jobs = (dh_crop_job*)malloc(rows * sizeof(dh_crop_job));
  int32_t* status = (int32_t*)malloc(rows * 4);
  rc = dh_refine_frames_host(plan, frames, src, boxes, n, OH, OW, outidx, num_iter, winsize_scale, momentum, poses, jobs, status);
  if (rc != DH_OK) { fprintf(stderr, "dh_refine_frames_host: %s\n", dh_error_string(rc)); return 1; }
  for (int t = 0; t < num_iter; ++t)
    for (int i = 0; i < n; ++i) {
      const dh_crop_job* g = jobs + (size_t)t * (size_t)n + (size_t)i;
      printf("window %d %d %d %d %d %d %d\n", t, i, g->x0, g->y0, g->x1, g->y1, status[(size_t)t * (size_t)n + (size_t)i]);
    }
  printf("%d samples, %d iterations, %d joints of %d channels\n", n, num_iter, J, dh_plan_output_channels(plan, outidx));
  if (dump(argv[12], "poses.f32", poses, rows * items * 4) || dump(argv[12], "jobs.i32", jobs, rows * sizeof(dh_crop_job)) ||
      dump(argv[12], "status.i32", status, rows * 4))
    return 2;
  dh_frames_destroy(frames);
  dh_plan_destroy(plan);
  return 0;
}
