/* A host WITHOUT Python that predicts from FULL frames and boxes: a uint8 plan exported by
 * deephar_amd.Model.export_plan(path, batch, uint8=True), fed through dh_frames_* / dh_forward_frames_host of
 * include/deephar_hip.h -- the frames are uploaded once, every crop-and-resize (the reference's per-frame PIL crop,
 * deephar/data/mpii.py:114-115) runs on the GPU straight into the plan's input.  Plain C, no HIP headers:
 *     gcc -O2 -Iinclude tools/c_host/predict_frames.c -Ldeephar_amd/csrc -ldeephar_hip -Wl,-rpath,$PWD/deephar_amd/csrc -o predict_frames
 *     ./predict_frames model.dhplan frames.u8 H W jobs.i32 OH OW out_prefix
 *   frames.u8 : raw uint8 [n, H, W, 3], n full frames of one size
 *   jobs.i32  : raw int32 [njobs, 6]: frame index, x0, y0, x1, y1, hflip (struct dh_crop_job); njobs = items x frames per item
 *   OH OW     : the crop size the model takes (the plan file does not carry it)
 * writes out_prefix.<k>.f32 per model output and prints the items/s of a second, timed call. */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
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

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s plan.dhplan frames.u8 H W jobs.i32 OH OW out_prefix\n", argv[0]); return 2; }
  const int H = atoi(argv[3]), W = atoi(argv[4]), OH = atoi(argv[6]), OW = atoi(argv[7]);
  size_t nb, nx, nj;
  void* blob = slurp(argv[1], &nb);
  uint8_t* px = (uint8_t*)slurp(argv[2], &nx);
  dh_crop_job* jobs = (dh_crop_job*)slurp(argv[5], &nj);
  if (H < 1 || W < 1 || nx == 0 || nx % ((size_t)H * (size_t)W * 3) != 0 || nj == 0 || nj % sizeof(dh_crop_job) != 0) {
    fprintf(stderr, "bad frame or job file size\n");
    return 1;
  }
  const int nframes = (int)(nx / ((size_t)H * (size_t)W * 3)), njobs = (int)(nj / sizeof(dh_crop_job));
  dh_plan* plan = NULL;
  int rc = dh_plan_create(blob, nb, &plan);
  if (rc != DH_OK) { fprintf(stderr, "dh_plan_create: %s\n", dh_error_string(rc)); return 1; }
  free(blob);
  int m = 0, per_item = 0;
  rc = dh_forward_frames_shape(dh_plan_num_inputs(plan), dh_plan_input_is_u8(plan, 0), dh_plan_input_items(plan, 0), dh_plan_batch(plan),
                               njobs, OH, OW, &m, &per_item);
  if (rc != DH_OK) { fprintf(stderr, "%d jobs of %d x %d do not fill this plan's uint8 input\n", njobs, OH, OW); return 1; }
  dh_crop_src* table = (dh_crop_src*)calloc((size_t)nframes, sizeof(dh_crop_src));
  for (int i = 0; i < nframes; ++i) {
    table[i].ptr = px + (size_t)i * (size_t)H * (size_t)W * 3;
    table[i].pitch = 3 * (int64_t)W;
    table[i].H = H;
    table[i].W = W;
  }
  dh_frames* frames = NULL;
  rc = dh_frames_create(table, nframes, &frames);
  if (rc != DH_OK) { fprintf(stderr, "dh_frames_create: %s\n", dh_error_string(rc)); return 1; }
  free(px);                                                   /* the frames live on the device now */
  free(table);
  const int nout = dh_plan_num_outputs(plan);
  float** outs = (float**)calloc((size_t)nout, sizeof(float*));
  for (int k = 0; k < nout; ++k) outs[k] = (float*)malloc((size_t)dh_plan_output_items(plan, k) * 4 * (size_t)m);
  rc = dh_forward_frames_host(plan, frames, jobs, njobs, OH, OW, outs);
  if (rc != DH_OK) { fprintf(stderr, "dh_forward_frames_host: %s\n", dh_error_string(rc)); return 1; }
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  rc = dh_forward_frames_host(plan, frames, jobs, njobs, OH, OW, outs);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  if (rc != DH_OK) return 1;
  for (int k = 0; k < nout; ++k) {
    char path[1024];
    snprintf(path, sizeof path, "%s.%d.f32", argv[8], k);
    FILE* f = fopen(path, "wb");
    if (!f) { perror(path); return 2; }
    fwrite(outs[k], 4, (size_t)dh_plan_output_items(plan, k) * (size_t)m, f);
    fclose(f);
  }
  const double dt = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  printf("%d frames resident, %d items of %d crop(s), %d outputs, %.3f ms (%.1f items/s incl. job upload / D2H)\n", nframes, m, per_item,
         nout, 1e3 * dt, m / dt);
  dh_frames_destroy(frames);
  dh_plan_destroy(plan);
  return 0;
}
