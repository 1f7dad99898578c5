/* A host WITHOUT Python that runs the per-frame person-box pass (exp/pennaction/predict_bboxes.py and exp/ntu/predict_bboxes.py in
 * the reference) over FULL frames: a uint8 plan exported by deephar_amd.Model.export_plan(path, batch, uint8=True), fed through
 * dh_frames_* / dh_frame_boxes_host of include/deephar_hip.h -- the frames are uploaded once, every frame is cropped with its
 * window and predicted on the GPU, the pose becomes a box there (dh_pose_boxes_f64), and only the boxes come back.  Plain C, no
 * HIP headers:
 *     gcc -O2 -Iinclude tools/c_host/frame_boxes.c -Ldeephar_amd/csrc -ldeephar_hip -Wl,-rpath,$PWD/deephar_amd/csrc -o frame_boxes
 *     ./frame_boxes model.dhplan frames.u8 H W windows.i32 OH OW outidx relsize out_prefix
 *   frames.u8   : raw uint8 [n, H, W, 3], n full frames of one size; sample i is frame i
 *   windows.i32 : raw int32 [n, 4], the unflipped crop windows (x0, y0, x1, y1); n <= the plan's batch
 *   OH OW       : the crop size the model takes (the plan file does not carry it)
 * writes out_prefix.boxes.i32 ([n, 4]), out_prefix.boxes.f64 ([n, 4]) and out_prefix.status.i32 ([n]), and prints every box:
 * "box <sample> x0 y0 x1 y1 status". */
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
  if (argc < 11) {
    fprintf(stderr, "usage: %s plan.dhplan frames.u8 H W windows.i32 OH OW outidx relsize out_prefix\n", argv[0]);
    return 2;
  }
  const int H = atoi(argv[3]), W = atoi(argv[4]), OH = atoi(argv[6]), OW = atoi(argv[7]), outidx = atoi(argv[8]);
  const double relsize = atof(argv[9]);
  size_t nb, nx, nwin;
  void* blob = slurp(argv[1], &nb);
  uint8_t* px = (uint8_t*)slurp(argv[2], &nx);
  int32_t* windows = (int32_t*)slurp(argv[5], &nwin);
  if (H < 1 || W < 1 || nx == 0 || nx % ((size_t)H * (size_t)W * 3) != 0 || nwin == 0 || nwin % 16 != 0 ||
      nwin / 16 != nx / ((size_t)H * (size_t)W * 3)) {
    fprintf(stderr, "bad frame or window file size (one window per frame)\n");
    free(blob);
    free(px);
    free(windows);
    return 1;
  }
  const int n = (int)(nwin / 16);
  /* everything this host owns, released on every way out (free(NULL) and the destroy calls on NULL do nothing) */
  dh_plan* plan = NULL;
  dh_frames* frames = NULL;
  dh_crop_src* table = (dh_crop_src*)calloc((size_t)n, sizeof(dh_crop_src));
  int32_t* src = (int32_t*)calloc((size_t)n, sizeof(int32_t));
  int32_t* boxes = (int32_t*)malloc((size_t)n * 16);
  double* boxes_f64 = (double*)malloc((size_t)n * 32);
  int32_t* status = (int32_t*)malloc((size_t)n * 4);
  int ret = 1, J = 0;
  int rc = DH_OK;
  if (!table || !src || !boxes || !boxes_f64 || !status) { fprintf(stderr, "out of memory\n"); goto done; }
  rc = dh_plan_create(blob, nb, &plan);
  if (rc != DH_OK) { fprintf(stderr, "dh_plan_create: %s\n", dh_error_string(rc)); goto done; }
  rc = dh_frame_boxes_shape(dh_plan_num_inputs(plan), dh_plan_input_is_u8(plan, 0), dh_plan_input_items(plan, 0), dh_plan_batch(plan), n,
                            OH, OW, dh_plan_num_outputs(plan), outidx, dh_plan_output_items(plan, outidx),
                            dh_plan_output_channels(plan, outidx), &J);
  if (rc != DH_OK) {
    fprintf(stderr, "this plan cannot box %d frames of %d x %d crops on output %d (single uint8 image input, a pose output)\n", n, OH, OW,
            outidx);
    goto done;
  }
  for (int i = 0; i < n; ++i) {
    table[i].ptr = px + (size_t)i * (size_t)H * (size_t)W * 3;
    table[i].pitch = 3 * (int64_t)W;
    table[i].H = H;
    table[i].W = W;
    src[i] = i;
  }
  rc = dh_frames_create(table, n, &frames);                   /* the frames live on the device from here on */
  if (rc != DH_OK) { fprintf(stderr, "dh_frames_create: %s\n", dh_error_string(rc)); goto done; }
  rc = dh_frame_boxes_host(plan, frames, src, windows, n, OH, OW, outidx, relsize, boxes, boxes_f64, status);
  if (rc != DH_OK) { fprintf(stderr, "dh_frame_boxes_host: %s\n", dh_error_string(rc)); goto done; }
  for (int i = 0; i < n; ++i)
    printf("box %d %d %d %d %d %d\n", i, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3], status[i]);
  printf("%d samples, %d joints of %d channels\n", n, J, dh_plan_output_channels(plan, outidx));
  ret = (dump(argv[10], "boxes.i32", boxes, (size_t)n * 16) || dump(argv[10], "boxes.f64", boxes_f64, (size_t)n * 32) ||
         dump(argv[10], "status.i32", status, (size_t)n * 4)) ? 2 : 0;
done:
  dh_frames_destroy(frames);
  dh_plan_destroy(plan);
  free(status);
  free(boxes_f64);
  free(boxes);
  free(src);
  free(table);
  free(windows);
  free(px);
  free(blob);
  return ret;
}
