// kv8_tail_probe.hip — the batched decode attention alone (launch_attn_decode_b), bf16 rows against the MXFP8 shadow, on the shapes of a
// 64-slot ds-7b / cl-7b step (32 heads, no GQA, 128-thread blocks): HIP events around back-to-back launches, the two formats
// alternating in one process.  Every launch of a burst reads another layer's planes (LAYERS distinct sets, far more bytes than the
// Infinity Cache holds), as the layers of a step do.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I detikzify_amd/csrc -c tools/probe/kv8_tail_probe.hip -o build/kv8_tail_probe.o
//   hipcc --offload-arch=gfx950 build/kv8_tail_probe.o build/kernels_batch_decode.o -o kv8_tail_probe      (after build.sh)
//   ./kv8_tail_probe [slots=64] [tail_threads=128]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels.h"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

// What kernels_batch_decode.o refers to in other units (never called here: they abort).  The list follows that unit: when it gains
// another external reference the link line above fails with the symbol's name, and its stub goes here.
int& dtk_lds_attr_error(int) { static int e = 0; return e; }
bool launch_gemv_bx(int, int, const GemvBArgs&, hipStream_t) { abort(); }
bool launch_gemv_bl(int, const GemvBArgs&, hipStream_t) { abort(); }
bool launch_gemv_bc(int, const GemvBArgs&, hipStream_t) { abort(); }
bool launch_gemv_bus(int, const GemvBArgs&, hipStream_t) { abort(); }

__global__ void k_fill_bf16(bf16_t* p, size_t n, unsigned seed) {      // values in (-2, 2)
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    const float f = ((int)(h & 0xffff) - 32768) * (1.f / 16384.f);
    p[i] = (bf16_t)(__float_as_uint(f) >> 16);
  }
}
__global__ void k_fill_u8(uint8_t* p, size_t n, unsigned seed, int lo, int span) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = (uint8_t)(lo + (int)(h % (unsigned)span));
  }
}

int main(int argc, char** argv) {
  const int NS = argc > 1 ? atoi(argv[1]) : 64, TT = argc > 2 ? atoi(argv[2]) : 128;
  const int H = 32, T_max = 1024, d = H * 128, LAYERS = 4, BURST = 8, REPS = 15, PFX = 243;
  const size_t slot_elems = (size_t)H * T_max * 128, plane = (size_t)NS * slot_elems;
  bf16_t *K[LAYERS], *V[LAYERS]; uint8_t *K8[LAYERS], *V8[LAYERS], *K8S[LAYERS], *V8S[LAYERS];
  for (int l = 0; l < LAYERS; ++l) {
    CHK(hipMalloc(&K[l], plane * 2)); CHK(hipMalloc(&V[l], plane * 2));
    CHK(hipMalloc(&K8[l], plane)); CHK(hipMalloc(&V8[l], plane)); CHK(hipMalloc(&K8S[l], plane / 32)); CHK(hipMalloc(&V8S[l], plane / 32));
    k_fill_bf16<<<4096, 256>>>(K[l], plane, 11u + l); k_fill_bf16<<<4096, 256>>>(V[l], plane, 23u + l);
    k_fill_u8<<<4096, 256>>>(K8[l], plane, 37u + l, 0, 0x78); k_fill_u8<<<4096, 256>>>(V8[l], plane, 41u + l, 0, 0x78);       // finite e4m3 codes
    k_fill_u8<<<1024, 256>>>(K8S[l], plane / 32, 43u + l, 118, 4); k_fill_u8<<<1024, 256>>>(V8S[l], plane / 32, 47u + l, 118, 4);
  }
  bf16_t *q, *out; DecState* st; BatchState* bs; float *pm, *pl, *po;
  const size_t out_elems = (size_t)((NS + 15) / 16) * ((d + 31) / 32) * 512, recs = (size_t)NS * H * 4;
  CHK(hipMalloc(&q, (size_t)NS * d * 2)); CHK(hipMalloc(&out, out_elems * 2)); CHK(hipMalloc(&st, sizeof(DecState) * NS)); CHK(hipMalloc(&bs, sizeof(BatchState)));
  CHK(hipMalloc(&pm, recs * 4)); CHK(hipMalloc(&pl, recs * 4)); CHK(hipMalloc(&po, recs * 128 * 4));
  k_fill_bf16<<<256, 256>>>(q, (size_t)NS * d, 5u);
  CHK(hipDeviceSynchronize());
  hipStream_t s; CHK(hipStreamCreate(&s));
  hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));

  // shared = 0: every slot walks [0, priv] alone (kv8_from 0).  shared = 1: slot 0 holds a PFX-row prefix and sits out; slots 1.. fork it
  // (prefix kernel on) and hold `priv` decoded rows behind it (kv8_from PFX).
  for (int shared = 0; shared < 2; ++shared)
    for (int priv : {4, 260, 480}) {
      std::vector<DecState> hst((size_t)NS); memset(hst.data(), 0, sizeof(DecState) * NS);
      BatchState hbs; memset(&hbs, 0, sizeof hbs);
      for (int j = 0; j < NS; ++j) {
        hst[j].pos = (shared ? PFX : 0) + priv; hst[j].next_pos = hst[j].pos + 1;
        hbs.active[j] = shared ? j > 0 : 1; hbs.share_src[j] = shared && j > 0 ? 0 : -1; hbs.share_len[j] = shared && j > 0 ? PFX : 0;
        hbs.kv8_from[j] = shared ? PFX : 0;
        if (shared && j > 0) {
          const int g = (j - 1) / 16;
          hbs.group_plus1[j] = g + 1; hbs.pfx_len_of[j] = PFX;
          PfxGroup& G = hbs.groups[g]; G.src = 0; G.len = PFX; G.slot[G.n++] = j;
          hbs.n_groups = std::max(hbs.n_groups, g + 1);
        }
      }
      for (int g = 0; g < hbs.n_groups; ++g) for (int i = hbs.groups[g].n; i < 16; ++i) hbs.groups[g].slot[i] = hbs.groups[g].slot[0];
      CHK(hipMemcpy(st, hst.data(), sizeof(DecState) * NS, hipMemcpyHostToDevice)); CHK(hipMemcpy(bs, &hbs, sizeof hbs, hipMemcpyHostToDevice));
      AttnDecBArgs a;
      a.q = q; a.kv_slot_stride = slot_elems; a.st = st; a.bs = bs; a.out = out; a.H = H; a.T_max = T_max; a.d = d; a.scale = 0.0883883f; a.G = 1;
      a.nslots = NS; a.use_prefix = shared; a.pfx_splits = 4; a.tail_threads = TT; a.gqa_fused = 1; a.nt_private = 1; a.pfx_m = pm; a.pfx_l = pl; a.pfx_o = po;
      a.kv8_slot_stride = slot_elems;
      auto burst = [&](bool kv8) {
        for (int i = 0; i < BURST; ++i) {
          const int l = i % LAYERS;
          a.kcache = K[l]; a.vcache = V[l];
          a.k8 = kv8 ? K8[l] : nullptr; a.v8 = kv8 ? V8[l] : nullptr; a.k8s = kv8 ? K8S[l] : nullptr; a.v8s = kv8 ? V8S[l] : nullptr;
          launch_attn_decode_b(a, s);
        }
      };
      burst(false); burst(true); CHK(hipStreamSynchronize(s));
      std::vector<float> t[2];
      for (int r = 0; r < REPS; ++r)
        for (int f = 0; f < 2; ++f) {
          CHK(hipEventRecord(e0, s)); burst(f != 0); CHK(hipEventRecord(e1, s)); CHK(hipEventSynchronize(e1));
          float ms = 0.f; CHK(hipEventElapsedTime(&ms, e0, e1)); t[f].push_back(ms * 1000.f / BURST);
        }
      CHK(hipGetLastError());
      for (int f = 0; f < 2; ++f) std::sort(t[f].begin(), t[f].end());
      printf("{\"slots\": %d, \"threads\": %d, \"shared_prefix\": %d, \"private_rows\": %d, \"bf16_us\": {\"min\": %.2f, \"median\": %.2f, \"max\": %.2f}, "
             "\"kv8_us\": {\"min\": %.2f, \"median\": %.2f, \"max\": %.2f}, \"ratio_median\": %.3f}\n", NS, TT, shared, priv,
             t[0].front(), t[0][REPS / 2], t[0].back(), t[1].front(), t[1][REPS / 2], t[1].back(), t[1][REPS / 2] / t[0][REPS / 2]);
      fflush(stdout);
    }
  return 0;
}
