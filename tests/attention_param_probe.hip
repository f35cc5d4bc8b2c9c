// CPU probe of the host layer in front of the flash-attention kernels: every entry point of open_sora_amd/csrc/attention_fwd.hip is
// called with well-formed fake-pointer arguments against STUB launch functions that record their AttnParams, and every launch is
// printed field by field (pointers as byte offsets from the argument they derive from).  One JSON object per line; the first names
// the fields.  tests/test_attention_entry_host.py compares the output with tests/golden/attention_launch_params.json
// (tools/make_golden_attention_launch_params.py builds and runs this file).
//
// Nothing here reaches a real launch: the asm launch functions and launch_merge_into are the stubs below, the CU count is 256 without
// asking a device, and the one launch attention_fwd.hip makes itself -- launch_merge after a tail split -- cannot happen: no call
// hands launch A a tail-split workspace, and a stub answers a parameter block with tail_split > 1 with a nonzero status anyway,
// which then_merge() returns without launching.
#include <cstdio>
#include <string>
#include <vector>
#include "../open_sora_amd/csrc/osk_common.h"
static int probe_device_cus() { return 256; }
#define osk_device_cus probe_device_cus
#include "../open_sora_amd/csrc/attention_fwd.hip"
#undef osk_device_cus

namespace {

// fake argument addresses, 16-byte aligned and 256 MiB apart: a derived pointer is printed as "<argument>+<bytes>"
struct Base { const char* name; uintptr_t addr; };
constexpr uintptr_t SPAN = 0x10000000;
const Base Q{"q", 1 * SPAN}, K{"k", 2 * SPAN}, VT{"vt", 3 * SPAN}, OUT{"out", 4 * SPAN}, LSE{"lse", 5 * SPAN}, WS{"ws", 6 * SPAN},
    KSCALE{"k_scale", 7 * SPAN}, VSCALE{"v_scale", 8 * SPAN}, QN2{"qn2", 9 * SPAN}, KN2{"kn2", 10 * SPAN}, WIN{"win", 11 * SPAN};
const Base* const BASES[] = {&Q, &K, &VT, &OUT, &LSE, &WS, &KSCALE, &VSCALE, &QN2, &KN2, &WIN};

template <class T = void>
T* at(const Base& b) { return reinterpret_cast<T*>(b.addr); }

std::string ptr(const void* p) {
  if (!p) return "null";
  const uintptr_t a = (uintptr_t)p;
  for (const Base* b : BASES)
    if (a >= b->addr && a < b->addr + SPAN) return std::string(b->name) + "+" + std::to_string(a - b->addr);
  return "stray";
}

std::vector<std::string> g_launches;

const char* const FIELDS =
    "\"kernel\", \"q\", \"qbs\", \"qrs\", \"k\", \"kss\", \"kbs\", \"krs\", \"vt\", \"vtss\", \"out\", \"obs\", \"ors\", \"lse\", \"B\", \"H\", \"Lq\", "
    "\"n_seg\", \"seg_len\", \"seg_lp\", \"tps\", \"sc\", \"bound\", \"q_prescaled\", \"rows\", \"Bkv\", \"map\", \"tail_first\", \"tail_split\", "
    "\"ws_o\", \"ws_lse\", \"vt8\", \"v_scale\", \"k8\", \"k_scale\", \"qn2\", \"kn2\", \"win\"";

int record(const std::string& kernel, const AttnParams& p) {
  char buf[1024];
  snprintf(buf, sizeof buf,
           "[\"%s\", \"%s\", %lld, %lld, \"%s\", %lld, %lld, %lld, \"%s\", %lld, \"%s\", %lld, %lld, \"%s\", %d, %d, %d, %d, %d, %d, %d, %.9g, %.9g, "
           "%d, %d, %d, %d, %d, %d, \"%s\", \"%s\", \"%s\", \"%s\", \"%s\", \"%s\", \"%s\", \"%s\", \"%s\"]",
           kernel.c_str(), ptr(p.q).c_str(), (long long)p.qbs, (long long)p.qrs, ptr(p.k).c_str(), (long long)p.kss, (long long)p.kbs,
           (long long)p.krs, ptr(p.vt).c_str(), (long long)p.vtss, ptr(p.out).c_str(), (long long)p.obs, (long long)p.ors, ptr(p.lse).c_str(),
           p.B, p.H, p.Lq, p.n_seg, p.seg_len, p.seg_lp, p.tps, p.sc, p.bound, p.q_prescaled, p.rows, p.Bkv, p.map, p.tail_first, p.tail_split,
           ptr(p.ws_o).c_str(), ptr(p.ws_lse).c_str(), ptr(p.vt8).c_str(), ptr(p.v_scale).c_str(), ptr(p.k8).c_str(), ptr(p.k_scale).c_str(),
           ptr(p.qn2).c_str(), ptr(p.kn2).c_str(), ptr(p.win).c_str());
  g_launches.push_back(buf);
  return p.tail_split > 1 ? 1 : 0;   // (never met: see the head of the file)
}

}  // namespace

namespace osk_attn {
int launch_asm72(const AttnParams& p, hipStream_t) { return record("asm72", p); }
int launch_asm72w(const AttnParams& p, hipStream_t) { return record("asm72w", p); }
int launch_asm64(const AttnParams& p, hipStream_t) { return record("asm64", p); }
int launch_asm64w(const AttnParams& p, hipStream_t) { return record("asm64w", p); }
int launch_asm128(const AttnParams& p, hipStream_t) { return record("asm128", p); }
int launch_asm128p8(const AttnParams& p, hipStream_t) { return record("asm128p8", p); }
int launch_asm72p8(const AttnParams& p, hipStream_t) { return record("asm72p8", p); }
int launch_asm128q8(const AttnParams& p, hipStream_t) { return record("asm128q8", p); }
int launch_merge_into(const AttnParams& p, int hd, float lse_b_mult, hipStream_t) {
  char name[64];
  snprintf(name, sizeof name, "merge_into hd=%d lse_b_mult=%.9g", hd, lse_b_mult);
  return record(name, p);
}
}  // namespace osk_attn

namespace {

void report(const std::string& call, int status) {
  printf("{\"call\": \"%s\", \"status\": %d, \"launches\": [", call.c_str(), status);
  for (size_t i = 0; i < g_launches.size(); ++i) printf("%s\n  %s", i ? "," : "", g_launches[i].c_str());
  printf("]}\n");
  g_launches.clear();
}

// the dimensions every call shares: B = 2, H = 2, 130 query rows (one 256-row block), tensors [B, L, H * hd] with their natural strides
constexpr int B = 2, H = 2, LQ = 130;
constexpr float SCALE = 0.125f, BOUND = 12.0f;
int rp(int hd) { return (hd + 1 + 15) / 16 * 16; }          // rows per head of the e4m3 V^T
int lp(int l) { return (l + 63) / 64 * 64; }
int64_t partial_bytes(int lq, int hd) { return (int64_t)((lq + 255) / 256) * B * H * 256 * (hd + 1) * 4; }
int64_t lse_bytes(int lq) { return ((int64_t)B * H * lq * 4 + 15) & ~(int64_t)15; }

struct Opt { bool lse; int kvb; };
std::string tag(const char* entry, int hd, Opt o, const std::string& more = "") {
  return std::string(entry) + " hd=" + std::to_string(hd) + (o.lse ? " lse" : " no-lse") + " kv_batches=" + std::to_string(o.kvb) + more;
}

// plain entries: n_seg = 2 segments of L keys, a segment = a [Bkv, L, H * hd] tensor (bf16), [Bkv, H, lp(L), 128] bytes (e4m3 K),
// [Bkv, H, hd | rp(hd), lp(L)] (V^T).  L = 200: 4 tiles per segment, so the FAST body is legal and auto launches its pair
void plain(int hd, Opt o, bool qk8 = false, int lq = LQ, int H = ::H, float bound = BOUND, int L = 200) {
  const int C = H * hd, Bkv = o.kvb ? o.kvb : B, n_seg = 2;
  const int64_t kss = (int64_t)Bkv * L * C, kbs = (int64_t)L * C, vtss = (int64_t)Bkv * H * hd * lp(L), vt8ss = (int64_t)Bkv * H * rp(hd) * lp(L);
  float* lse = o.lse ? at<float>(LSE) : nullptr;
  if (qk8) {
    report(tag("qk8", hd, o), osk_attention_fwd_qk8_bf16(at(Q), (int64_t)lq * C, C, at(K), (int64_t)Bkv * H * lp(L) * 128, (int64_t)H * lp(L) * 128, 128,
                                                         at<float>(KSCALE), at(VT), vt8ss, at<float>(VSCALE), at(OUT), (int64_t)lq * C, C, lse, B, H, lq,
                                                         n_seg, L, hd, SCALE, 1, o.kvb, nullptr, 0, nullptr));
    return;
  }
  const std::string more = (lq == LQ ? "" : " Lq=" + std::to_string(lq) + " H=" + std::to_string(H) + " bound=" + std::to_string((int)bound)) +
                           (L == 200 ? "" : " seg_len=" + std::to_string(L));
  report(tag("bounded", hd, o, more), osk_attention_fwd_bounded_bf16(at(Q), (int64_t)lq * C, C, at(K), kss, kbs, C, at(VT), vtss, at(OUT), (int64_t)lq * C,
                                                                     C, lse, B, H, lq, n_seg, L, hd, SCALE, 1, o.kvb, bound, nullptr, 0, nullptr));
  if (lq != LQ) return;
  report(tag("auto", hd, o, more), osk_attention_fwd_auto_bf16(at(Q), (int64_t)lq * C, C, at(K), kss, kbs, C, at(VT), vtss, at(OUT), (int64_t)lq * C, C, lse, B,
                                                         H, lq, n_seg, L, hd, SCALE, 1, o.kvb, at<float>(QN2), at<float>(KN2), nullptr, 0, nullptr));
  if (hd != 64)
    report(tag("pv8", hd, o, more), osk_attention_fwd_pv8_bf16(at(Q), (int64_t)lq * C, C, at(K), kss, kbs, C, at(VT), vt8ss, at<float>(VSCALE), at(OUT),
                                                         (int64_t)lq * C, C, lse, B, H, lq, n_seg, L, hd, SCALE, 1, o.kvb, nullptr, 0, nullptr));
}

// ragged entry: n_seg = 3 segments of 100 keys (128 positions), the last holds 40 (64 positions: a packed K batch stride of its own).  The workspace is exactly the partials (+ the borrowed lse): launch
// A's share is empty, so it gets no tail split
void ragged(int hd, int mode, Opt o) {
  const int C = H * hd, Bkv = o.kvb ? o.kvb : B, L = 100;
  const bool k8 = mode == OSK_ATTN_QK8, v8 = mode != OSK_ATTN_BF16;
  const int64_t kss = k8 ? (int64_t)Bkv * H * lp(L) * 128 : (int64_t)Bkv * L * C, kbs = k8 ? (int64_t)H * lp(L) * 128 : (int64_t)L * C;
  const int64_t vtss = (int64_t)Bkv * H * (v8 ? rp(hd) : hd) * lp(L);
  const char* names[] = {"ragged bf16", "ragged pv8", "ragged qk8"};
  report(tag(names[mode], hd, o),
         osk_attention_fwd_ragged_bf16(at(Q), (int64_t)LQ * C, C, at(K), kss, kbs, k8 ? 128 : C, k8 ? at<float>(KSCALE) : nullptr, at(VT), vtss,
                                       v8 ? at<float>(VSCALE) : nullptr, at(OUT), (int64_t)LQ * C, C, o.lse ? at<float>(LSE) : nullptr, B, H, LQ, 3, L, 40,
                                       hd, SCALE, 1, o.kvb, v8 ? 0.f : BOUND, mode, at(WS), partial_bytes(LQ, hd) + (o.lse ? 0 : lse_bytes(LQ)), nullptr));
}

// window entries: Lk = 128 keys, n_prefix of them the prefix; the workspace the entry asks for, none with n_prefix = 0
void window(int hd, int mode, Opt o, int n_prefix) {
  const int C = H * hd, LK = 128;
  const bool k8 = mode == OSK_ATTN_QK8;
  const int64_t kbs = k8 ? (int64_t)H * lp(LK) * 128 : (int64_t)LK * C, krs = k8 ? 128 : C;
  float* lse = o.lse ? at<float>(LSE) : nullptr;
  void* ws = n_prefix ? at(WS) : nullptr;
  const int64_t ws_bytes = n_prefix ? osk_attention_window_workspace_bytes(B, H, LQ, hd) : 0;
  const std::string more = " n_prefix=" + std::to_string(n_prefix);
  if (mode == OSK_ATTN_BF16)
    report(tag("window", hd, o, more),
           osk_attention_fwd_window_bf16(at(Q), (int64_t)LQ * C, C, at(K), kbs, krs, at(VT), at(OUT), (int64_t)LQ * C, C, lse, B, H, LQ, LK, n_prefix, hd,
                                         SCALE, 1, o.kvb, BOUND, at<int32_t>(WIN), 1, ws, ws_bytes, nullptr));
  else
    report(tag(k8 ? "window_fp8 qk8" : "window_fp8 pv8", hd, o, more),
           osk_attention_fwd_window_fp8_bf16(at(Q), (int64_t)LQ * C, C, at(K), kbs, krs, k8 ? at<float>(KSCALE) : nullptr, at(VT), at<float>(VSCALE), at(OUT),
                                             (int64_t)LQ * C, C, lse, B, H, LQ, LK, n_prefix, hd, SCALE, 1, o.kvb, mode, at<int32_t>(WIN), 1, ws, ws_bytes,
                                             nullptr));
}

}  // namespace

int main() {
  printf("{\"fields\": [%s]}\n", FIELDS);
  const Opt opts[] = {{true, 0}, {false, 0}, {true, 1}, {false, 1}};
  // every entry and mode at its smallest head dim (bf16: 72, the dim every entry has; 64 and 128 below), lse given and not, kv_batches 0 and 1
  for (Opt o : opts) {
    plain(72, o);
    plain(128, o, true);
    ragged(72, OSK_ATTN_BF16, o);
    ragged(72, OSK_ATTN_PV8, o);
    ragged(128, OSK_ATTN_QK8, o);
    for (int n_prefix : {0, 64}) {
      window(72, OSK_ATTN_BF16, o, n_prefix);
      window(72, OSK_ATTN_PV8, o, n_prefix);
      window(128, OSK_ATTN_QK8, o, n_prefix);
    }
  }
  // the other head dims: hd 64 and 128 of the bf16 operands (with 128: pv8 too)
  for (int hd : {64, 128}) {
    plain(hd, opts[0]);
    ragged(hd, OSK_ATTN_BF16, opts[0]);
    if (hd == 128) ragged(hd, OSK_ATTN_PV8, opts[0]);
    for (int n_prefix : {0, 64}) {
      window(hd, OSK_ATTN_BF16, opts[0], n_prefix);
      if (hd == 128) window(hd, OSK_ATTN_PV8, opts[0], n_prefix);
    }
  }
  // a bounded call that takes the wide layout (512-row units), and the same without a bound (the general body: 256-row units)
  plain(72, opts[0], false, 2048, 32, BOUND);
  plain(72, opts[0], false, 2048, 32, 0.f);
  // segments of 2 tiles: only the general body takes them (auto: one launch, no pair)
  plain(72, opts[0], false, LQ, H, BOUND, 100);
  // the two older names of the bounded entry
  const int C = H * 72;
  report("fwd hd=72", osk_attention_fwd_bf16(at(Q), (int64_t)LQ * C, C, at(K), 0, (int64_t)100 * C, C, at(VT), 0, at(OUT), (int64_t)LQ * C, C, nullptr, B, H,
                                             LQ, 1, 100, 72, SCALE, 0, 0, nullptr));
  report("fwd_ws hd=72", osk_attention_fwd_ws_bf16(at(Q), (int64_t)LQ * C, C, at(K), 0, (int64_t)100 * C, C, at(VT), 0, at(OUT), (int64_t)LQ * C, C, nullptr, B,
                                                   H, LQ, 1, 100, 72, SCALE, 0, 0, nullptr, 0, nullptr));
  return 0;
}
