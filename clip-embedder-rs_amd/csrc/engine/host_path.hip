// The host-buffer entry points: caller-registered host ranges, the chunked and double-buffered
// host-buffer pipeline, and the decoded-image (crop / resize on the GPU) pipeline.
#include "engine.hpp"

namespace clipgpu {

namespace {

// Caller-registered host ranges (clipgpu_host_register): process-wide, hipHostRegister'ed.
constexpr size_t kHostPage = 4096;
struct HostRanges {
  std::mutex mu;
  std::vector<std::pair<uintptr_t, size_t>> r;  // (base, bytes)
};
HostRanges& host_ranges() {
  static HostRanges h;
  return h;
}
// Is [p, p + n) inside one registered range?
bool host_registered(const void* p, size_t n) {
  HostRanges& h = host_ranges();
  std::lock_guard<std::mutex> lk(h.mu);
  const uintptr_t a = (uintptr_t)p;
  for (const auto& rg : h.r)
    if (a >= rg.first && a + n <= rg.first + rg.second) return true;
  return false;
}

// The fixed partition of a round's max_batch rows into host-path chunks: part[0] = 0 < part[1] <
// ... < part[C] = MB, `lanes` even chunks.  Measured on the bench's ViT-B/32 u8 batch of 256
// (tools/host_plan_ab.py, profiles/r04_host_plan_ab.jsonl): two halves beat a small first chunk
// (64 or 96 rows) and three- or four-chunk plans, whose small forwards run far below the full
// batch's rate.
std::vector<int> host_chunks(const clipgpu_engine& e, InKind kind) {
  const int MB = e.max_batch, L = e.lanes;
  if (!e.host_part.empty() && kind != IN_IDS) return e.host_part;
  std::vector<int> part{0};
  for (int i = 1; i < L; ++i) part.push_back((int)(((long)MB * i + L - 1) / L));
  part.push_back(MB);
  return part;
}

// The second host-path buffer set of a replica (multi-round host calls), allocated once.
void ensure_host_set2(const clipgpu_engine& e, Replica& r) {
  HostSet& hs = r.hset[1];
  if (hs.in) return;
  const size_t B = (size_t)((e.max_batch + e.lanes - 1) / e.lanes * e.lanes);
  hs.owns_device = true;
  HIP_CHECK(hipMalloc(&hs.in, B * e.in_bytes_per_row));
  HIP_CHECK(hipHostMalloc(&hs.pin_in, B * e.in_bytes_per_row, hipHostMallocDefault));
  HIP_CHECK(hipHostMalloc((void**)&hs.pin_out, B * (size_t)e.spec.embed_dim * 4, hipHostMallocDefault));
  HIP_CHECK(hipMalloc((void**)&hs.out, B * (size_t)e.spec.embed_dim * 4));
  for (int i = 0; i < 4; ++i) {
    HIP_CHECK(hipEventCreateWithFlags(&hs.done[i], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&hs.copied[i], hipEventDisableTiming));
  }
}

// Host-buffer forward over a row range of one replica.  Each round of up to max_batch rows is cut
// by host_chunks' partition; chunk k of a round uses rows [part[k], part[k + 1]) of the
// max_batch-row device buffers, workspace (lane_view) and pinned staging, so chunks of one round
// never share memory and chunk k of the next round reuses only chunk k's rows, after chunk k's D2H
// event.  The H2Ds go in chunk order on the replica's copy stream (the first chunk gets the whole
// link); chunk k's forward runs on lane stream k % lanes once its copy event has fired, so the
// transfer of chunk k + 1 overlaps the forward of chunk k, and forwards of different lanes
// overlap each other.  Inputs are DMA'd straight from a caller-registered range
// (clipgpu_host_register) or staged through pinned memory by the copy pool in pieces of whole rows
// (kStagePiece), each piece's H2D issued as soon as it is packed, so a chunk's transfer runs under the
// packing of its later pieces; outputs are written straight into a registered range, or staged.
// A range of more than max_batch rows alternates its rounds between two buffer sets (device input
// rows, pinned staging, events): round i's host copy and H2D are issued while round i - 1's forward
// runs, and a set is reused two rounds later, after its round's D2H event -- so every round but the
// first starts its forward with its input already on the device.  Each set also
// has its own device embedding rows, copied back on the second copy stream once the forward has ended,
// so a lane's next forward starts right behind its last one.  Each round runs the same forward on the
// same rows as a call of its own: the outputs are bit-identical.
// (Round 6 removed the schedules measured and not kept -- lockstep, joined and device-path rounds, D2H
// on the copy or lane streams, split and pulled H2Ds; DESIGN.md §10 keeps their numbers.)
constexpr size_t kStagePiece = 4u << 20;

void run_host_shard(clipgpu_engine& e, Replica& r, InKind kind, const HostRows& src, int64_t b0, int64_t b1,
                    const float* mean, const float* stdv, float* out, int tokens = 0) {
  HIP_CHECK(hipSetDevice(r.device));
  const int E = e.spec.embed_dim, L = e.lanes, MB = e.max_batch;
  const size_t rb = src.row_bytes;
  const bool direct_in = src.rows == nullptr && host_registered(src.in + b0 * rb, (size_t)(b1 - b0) * rb);
  const bool direct_out = host_registered(out + b0 * E, (size_t)(b1 - b0) * E * 4);
  const std::vector<int> part = host_chunks(e, kind);
  const int C = (int)part.size() - 1;
  const bool two_sets = b1 - b0 > MB;
  if (two_sets) ensure_host_set2(e, r);
  struct Pending { int64_t c0 = -1; int n = 0; };
  Pending pend[2][4];
  auto drain = [&](int set, int k) {
    if (pend[set][k].c0 < 0) return;
    HIP_CHECK(hipEventSynchronize(r.hset[set].done[k]));
    if (!direct_out)
      std::memcpy(out + pend[set][k].c0 * E, r.hset[set].pin_out + (size_t)part[k] * E,
                  (size_t)pend[set][k].n * E * 4);
    pend[set][k].c0 = -1;
  };
  const int rows_per_piece = (int)std::max<size_t>(1, kStagePiece / rb);
  int round = 0;
  for (int64_t c0 = b0; c0 < b1; ++round) {
    const int set = two_sets ? (round & 1) : 0;
    HostSet& hs = r.hset[set];
    const int R = (int)std::min<int64_t>(MB, b1 - c0);  // rows of this round
    int off = 0;
    for (int k = 0; k < C && off < R; ++k) {
      const int cap = part[k + 1] - part[k];
      // a round of at least half of max_batch spreads over the chunks in proportion to the
      // partition; a shorter one fills them in order (a small batch is one forward)
      int n = 2 * R < MB ? R - off
              : k + 1 == C ? R - off : (int)(((long)R * part[k + 1] + MB - 1) / MB - off);
      n = std::max(0, std::min(n, cap));
      if (n == 0) continue;
      const int64_t rc = c0 + off;
      drain(set, k);  // this set's round before last: its D2H (so also its H2D and forward) done
      hipStream_t st = r.lane[k % L] ? r.lane[k % L] : r.stream;
      char* din = (char*)hs.in + (size_t)part[k] * rb;
      float* dout = hs.out + (size_t)part[k] * E;
      if (direct_in) {
        HIP_CHECK(hipMemcpyAsync(din, src.in + rc * rb, (size_t)n * rb, hipMemcpyHostToDevice, r.copy));
      } else {
        char* pin = (char*)hs.pin_in + (size_t)part[k] * rb;
        for (int p0 = 0; p0 < n; p0 += rows_per_piece) {
          const int pn = std::min(rows_per_piece, n - p0);
          char* pp = pin + (size_t)p0 * rb;
          if (src.rows) pool_gather(pp, src.rows + rc + p0, rb, pn);
          else pool_memcpy(pp, src.in + (rc + p0) * rb, (size_t)pn * rb);
          HIP_CHECK(hipMemcpyAsync(din + (size_t)p0 * rb, pp, (size_t)pn * rb, hipMemcpyHostToDevice, r.copy));
        }
      }
      HIP_CHECK(hipEventRecord(hs.copied[k], r.copy));
      HIP_CHECK(hipStreamWaitEvent(st, hs.copied[k], 0));
      const Replica v = lane_view(e, r, part[k]);
      run_graph(e, r,
                {(uint64_t)(10 + kind), (uint64_t)k, (uint64_t)n, fbits(mean, 0), fbits(mean, 1), fbits(mean, 2),
                 fbits(stdv, 0), fbits(stdv, 1), fbits(stdv, 2), (uint64_t)tokens, (uint64_t)part[k], (uint64_t)set,
                 (uint64_t)(uintptr_t)dout},
                st, [&](hipStream_t gs) {
                  if (kind == IN_IDS)
                    text_forward(e, v, (const int64_t*)din, n, dout, gs, tokens);
                  else
                    vision_forward(e, v, din, kind == IN_F32 ? A_IMG_F32 : A_IMG_U8, mean, stdv, n, dout, gs);
                });
      float* dst = direct_out ? out + rc * E : hs.pin_out + (size_t)part[k] * E;
      if (two_sets) {  // the forward's end, then the D2H on the second copy stream
        HIP_CHECK(hipEventRecord(hs.done[k], st));
        HIP_CHECK(hipStreamWaitEvent(r.copy2, hs.done[k], 0));
        HIP_CHECK(hipMemcpyAsync(dst, dout, (size_t)n * E * 4, hipMemcpyDeviceToHost, r.copy2));
        HIP_CHECK(hipEventRecord(hs.done[k], r.copy2));
      } else {
        HIP_CHECK(hipMemcpyAsync(dst, dout, (size_t)n * E * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipEventRecord(hs.done[k], st));
      }
      pend[set][k].c0 = rc;
      pend[set][k].n = n;
      off += n;
    }
    c0 += R;
  }
  for (int set = 0; set < 2; ++set)
    for (int k = 0; k < C; ++k) drain(set, k);
}

// Contiguous row blocks over the replicas (rank order == input order), one host thread each.
template <typename F>
void run_sharded(clipgpu_engine& e, int64_t B, F shard) {
  const int G = (int)e.reps.size();
  if (G == 1) {
    shard(e.reps[0], (int64_t)0, B);
    return;
  }
  std::vector<std::thread> th;
  std::vector<std::string> errs(G);
  std::vector<int> codes(G, 0);
  for (int g = 0; g < G; ++g) {
    const int64_t b0 = B * g / G, b1 = B * (g + 1) / G;
    if (b0 == b1) continue;
    th.emplace_back([&, g, b0, b1]() {
      try {
        shard(e.reps[g], b0, b1);
      } catch (const ClipErr& ex) {
        codes[g] = ex.code;
        errs[g] = ex.what();
      } catch (const std::exception& ex) {
        codes[g] = CLIPGPU_ERR_DEVICE;
        errs[g] = ex.what();
      }
    });
  }
  for (auto& t : th) t.join();
  for (int g = 0; g < G; ++g)
    if (codes[g]) throw ClipErr(codes[g], "device " + std::to_string(e.reps[g].device) + ": " + errs[g]);
}

void run_host(clipgpu_engine& e, InKind kind, const HostRows& src, int64_t B, const float* mean, const float* stdv,
              float* out, int tokens = 0) {
  run_sharded(e, B, [&](Replica& r, int64_t b0, int64_t b1) {
    run_host_shard(e, r, kind, src, b0, b1, mean, stdv, out, tokens);
  });
}

// ---- decoded RGB8 images -> embeddings, crop/resize on the GPU -------------------------
// Host: per image a ResizePlan (the same fixed-point tables as the host resize); device:
// launch_resize into the slot's u8 NHWC input rows, then the u8 vision forward (normalise
// + patch rows + trunk).  Chunks of <= one lane's rows (and <= kChunkRawBytes of source
// pixels) pipelined over the lane slots as run_host_shard does.
constexpr size_t kChunkRawBytes = 256u << 20;

// The staged source of an image is only the window its resize reads (round 6): the horizontal pass reads
// source rows [yfirst, yfirst + th) and, over all its outputs, columns [x0, x1) -- a 640x480 image cropped
// to its centre square needs 486 of its 640 columns; a vertical-only plan (width already S) reads rows
// [y0, y1).  The descriptor and the tap bounds are shifted to the window, so every output reads the same
// pixels with the same coefficients (bit-identical to the host resize).
struct ResizeBatch {
  std::vector<ResizeImage> d;
  std::vector<int> ints;
  std::vector<size_t> raw_off;  // per image, in the raw region
  struct Window { int y0, rows, x0, cols; };
  std::vector<Window> win;      // per image: the source window staged
  size_t raw_bytes = 0, tmp_bytes = 0;
  int max_th = 0;
};

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

ResizeBatch plan_resize_batch(int S, const std::string& interp, const std::string& mode, const int* W, const int* H,
                              int64_t i0, int n) {
  ResizeBatch b;
  b.d.resize(n);
  b.raw_off.resize(n);
  b.win.resize(n);
  for (int i = 0; i < n; ++i) {
    const ResizePlan p = make_resize_plan(W[i0 + i], H[i0 + i], S, interp, mode);
    ResizeImage& d = b.d[i];
    d.W = p.W;
    d.th = p.need_h ? p.th : 0;
    d.yfirst = p.yfirst;
    d.need_h = p.need_h;
    d.need_v = p.need_v;
    d.h_ksize = p.h.ksize;
    d.v_ksize = p.v.ksize;
    d.h_prec = p.h.prec;
    d.v_prec = p.v.prec;
    auto put = [&](const std::vector<int>& v) {
      const long off = (long)b.ints.size();
      b.ints.insert(b.ints.end(), v.begin(), v.end());
      return off;
    };
    ResizeBatch::Window w{0, p.H, 0, p.W};
    std::vector<int> hb = p.h.bounds, vb = p.v.bounds;
    if (p.need_h && p.th > 0 && !hb.empty()) {  // rows [yfirst, yfirst + th), the columns the taps read
      int x0 = hb[0], x1 = hb[0] + hb[1];
      for (size_t o = 0; o + 1 < hb.size(); o += 2) {
        x0 = std::min(x0, hb[o]);
        x1 = std::max(x1, hb[o] + hb[o + 1]);
      }
      for (size_t o = 0; o < hb.size(); o += 2) hb[o] -= x0;
      w = {p.yfirst, p.th, x0, x1 - x0};
      d.W = w.cols;
      d.yfirst = 0;
    } else if (!p.need_h && p.need_v && !vb.empty()) {  // the rows the vertical taps read, all S columns
      int y0 = vb[0], y1 = vb[0] + vb[1];
      for (size_t o = 0; o + 1 < vb.size(); o += 2) {
        y0 = std::min(y0, vb[o]);
        y1 = std::max(y1, vb[o] + vb[o + 1]);
      }
      for (size_t o = 0; o < vb.size(); o += 2) vb[o] -= y0;
      w = {y0, y1 - y0, 0, p.W};
    }
    b.win[i] = w;
    d.h_bounds = put(hb);
    d.h_coef = put(std::vector<int>(p.h.k.begin(), p.h.k.end()));
    d.v_bounds = put(vb);
    d.v_coef = put(std::vector<int>(p.v.k.begin(), p.v.k.end()));
    b.raw_off[i] = b.raw_bytes;
    d.src = (long)b.raw_bytes;  // relative to the raw region
    b.raw_bytes = align16(b.raw_bytes + (size_t)w.rows * w.cols * 3);
    d.tmp = (long)b.tmp_bytes;
    if (p.need_h) b.tmp_bytes = align16(b.tmp_bytes + (size_t)p.th * S * 3);
    b.max_th = std::max(b.max_th, d.th);
  }
  return b;
}

// Copy tasks that stage image i's window (src: its full [H][W][3] pixels, W its width) at dst.
void add_window_tasks(std::vector<CopyTask>& t, const ResizeBatch& b, int i, char* dst, const uint8_t* src, int W) {
  const ResizeBatch::Window& w = b.win[i];
  add_copy_tasks_2d(t, dst, src + ((size_t)w.y0 * W + w.x0) * 3, (size_t)w.cols * 3, (size_t)w.rows, (size_t)W * 3);
}

void grow_pinned(char*& p, size_t& cap, size_t need) {
  if (need <= cap) return;
  if (p) HIP_CHECK(hipHostFree(p));
  p = nullptr;
  cap = 0;
  HIP_CHECK(hipHostMalloc((void**)&p, need, hipHostMallocDefault));
  cap = need;
}
template <typename P>
void grow_device(P*& p, size_t& cap, size_t need) {
  if (need <= cap) return;
  if (p) HIP_CHECK(hipFree(p));
  p = nullptr;
  cap = 0;
  HIP_CHECK(hipMalloc((void**)&p, need));
  cap = need;
}

// Chunks alternate over the lane slots; per chunk: the resize plans' tables and the source images are
// packed into the slot's pinned staging by the copy pool, in pieces of whole images (kStagePiece) whose
// H2Ds go on the copy stream as soon as each is packed (round 6; round 5 spawned std::threads per chunk
// and ran the H2D on the lane stream), then on the lane: the resize kernels into the slot's u8 rows and
// the u8 forward.  The packing of chunk j + 1 runs while chunk j transfers and computes.
void run_images_shard(clipgpu_engine& e, Replica& r, const uint8_t* const* images, const int* W, const int* H,
                      int64_t b0, int64_t b1, float* out) {
  HIP_CHECK(hipSetDevice(r.device));
  const int E = e.spec.embed_dim, L = e.lanes, S = e.spec.image_size;
  const int rows = (e.max_batch + L - 1) / L;  // rows per slot
  HostSet& hs = r.hset[0];
  struct Pending { int64_t c0 = -1; int n = 0; };
  Pending pend[4];
  auto drain = [&](int k) {
    if (pend[k].c0 < 0) return;
    HIP_CHECK(hipEventSynchronize(hs.done[k]));
    std::memcpy(out + pend[k].c0 * E, hs.pin_out + (size_t)k * rows * E, (size_t)pend[k].n * E * 4);
    pend[k].c0 = -1;
  };
  int j = 0;
  for (int64_t c0 = b0; c0 < b1; ++j) {
    // chunk: up to `rows` images and kChunkRawBytes of source pixels (at least one image)
    int n = 0;
    size_t raw = 0;
    while (c0 + n < b1 && n < rows) {
      const size_t sz = (size_t)W[c0 + n] * H[c0 + n] * 3;
      if (n > 0 && raw + sz > kChunkRawBytes) break;
      raw += sz;
      ++n;
    }
    const int k = j % L;
    drain(k);  // slot k's previous chunk (its H2D, resize, forward and D2H) is done
    hipStream_t st = r.lane[k] ? r.lane[k] : r.stream;
    const ResizeBatch b = plan_resize_batch(S, e.pre.interpolation, e.pre.resize_mode, W, H, c0, n);
    const size_t desc_bytes = align16(b.d.size() * sizeof(ResizeImage));
    const size_t ints_bytes = align16(b.ints.size() * sizeof(int));
    const size_t head = desc_bytes + ints_bytes, total = head + b.raw_bytes;
    Replica::ImageSlot& sl = r.islot[k];
    grow_pinned(sl.pin, sl.pin_cap, total);
    grow_device(sl.dev, sl.dev_cap, total);
    grow_device(sl.tmp, sl.tmp_cap, std::max<size_t>(b.tmp_bytes, 16));
    std::memcpy(sl.pin, b.d.data(), b.d.size() * sizeof(ResizeImage));
    std::memcpy(sl.pin + desc_bytes, b.ints.data(), b.ints.size() * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(sl.dev, sl.pin, head, hipMemcpyHostToDevice, r.copy));
    char* const raw_pin = sl.pin + head;
    for (int i0 = 0; i0 < n;) {  // pieces of whole images
      int i1 = i0 + 1;
      while (i1 < n && b.raw_off[i1] - b.raw_off[i0] < kStagePiece) ++i1;
      const size_t p0 = b.raw_off[i0], p1 = i1 < n ? b.raw_off[i1] : b.raw_bytes;
      std::vector<CopyTask> tasks;
      for (int i = i0; i < i1; ++i) add_window_tasks(tasks, b, i, raw_pin + b.raw_off[i], images[c0 + i], W[c0 + i]);
      pool_copy(tasks);
      HIP_CHECK(hipMemcpyAsync(sl.dev + head + p0, raw_pin + p0, p1 - p0, hipMemcpyHostToDevice, r.copy));
      i0 = i1;
    }
    HIP_CHECK(hipEventRecord(hs.copied[k], r.copy));
    HIP_CHECK(hipStreamWaitEvent(st, hs.copied[k], 0));
    uint8_t* din = (uint8_t*)hs.in + (size_t)k * rows * e.in_bytes_per_row;  // u8 [n][S][S][3]
    check(launch_resize((const uint8_t*)sl.dev + head, sl.tmp, (const int*)(sl.dev + desc_bytes),
                        (const ResizeImage*)sl.dev, n, b.max_th, S, din, st), "resize");
    float* dout = hs.out + (size_t)k * rows * E;
    const Replica v = lane_view(e, r, k * rows);
    run_graph(e, r, {20, (uint64_t)k, (uint64_t)n}, st,
              [&](hipStream_t gs) { vision_forward(e, v, din, A_IMG_U8, e.pre.mean, e.pre.stdv, n, dout, gs); });
    HIP_CHECK(hipMemcpyAsync(hs.pin_out + (size_t)k * rows * E, dout, (size_t)n * E * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(hs.done[k], st));
    pend[k].c0 = c0;
    pend[k].n = n;
    c0 += n;
  }
  for (int k = 0; k < L; ++k) drain(k);
}

}  // namespace

}  // namespace clipgpu

using namespace clipgpu;

extern "C" {

int clipgpu_embed_pixels(clipgpu_engine* e, const float* nchw, int64_t B, int64_t S, float* out) {
  return guarded([&]() {
    need_tower(e, TOWER_VISION);
    if (B <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
    if (!nchw || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    if (S != e->spec.image_size)
      throw ClipErr(CLIPGPU_ERR_INVALID, "Shape error: expected image size " + std::to_string(e->spec.image_size));
    std::lock_guard<std::mutex> lk(e->mu);
    run_host(*e, IN_F32, HostRows{(const char*)nchw, nullptr, (size_t)3 * S * S * 4}, B, nullptr, nullptr, out);
  });
}

int clipgpu_embed_u8(clipgpu_engine* e, const uint8_t* nhwc, int64_t B, int64_t S, const float mean[3],
                     const float stdv[3], float* out) {
  return guarded([&]() {
    need_tower(e, TOWER_VISION);
    if (B <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
    if (!nhwc || !out || !mean || !stdv) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    if (S != e->spec.image_size)
      throw ClipErr(CLIPGPU_ERR_INVALID, "Shape error: expected image size " + std::to_string(e->spec.image_size));
    std::lock_guard<std::mutex> lk(e->mu);
    run_host(*e, IN_U8, HostRows{(const char*)nhwc, nullptr, (size_t)3 * S * S}, B, mean, stdv, out);
  });
}

int clipgpu_host_register(void* ptr, size_t bytes) {
  return guarded([&]() {
    if (!ptr || bytes == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL / empty host range");
    HostRanges& h = host_ranges();
    std::lock_guard<std::mutex> lk(h.mu);
    const uintptr_t a = (uintptr_t)ptr;
    for (const auto& rg : h.r)
      if (a < rg.first + rg.second && rg.first < a + bytes)
        throw ClipErr(CLIPGPU_ERR_INVALID, "host range overlaps a registered one");
    // hipHostRegister pins whole pages: two ranges that share a page would pin it twice, and unregistering
    // one would unpin it under the other (and leave the runtime's page mapping stale for whatever the
    // allocator puts there next).  Such a range is refused; page-owning buffers (engine.py host_buffer)
    // never share one.
    const uintptr_t pg = (uintptr_t)kHostPage;
    for (const auto& rg : h.r)
      if (a / pg <= (rg.first + rg.second - 1) / pg && rg.first / pg <= (a + bytes - 1) / pg)
        throw ClipErr(CLIPGPU_ERR_INVALID,
                      "host range shares a memory page with a registered one (registration pins whole pages): "
                      "register page-aligned buffers");
    HIP_CHECK(hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable));  // every device
    h.r.emplace_back(a, bytes);
  });
}

int clipgpu_host_unregister(void* ptr) {
  return guarded([&]() {
    HostRanges& h = host_ranges();
    std::lock_guard<std::mutex> lk(h.mu);
    for (size_t i = 0; i < h.r.size(); ++i)
      if (h.r[i].first == (uintptr_t)ptr) {
        // no transfer of any device may still reference the range
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        int cur = 0;
        HIP_CHECK(hipGetDevice(&cur));
        for (int d = 0; d < ndev; ++d) {
          HIP_CHECK(hipSetDevice(d));
          HIP_CHECK(hipDeviceSynchronize());
        }
        HIP_CHECK(hipSetDevice(cur));
        HIP_CHECK(hipHostUnregister(ptr));
        h.r.erase(h.r.begin() + (long)i);
        return;
      }
    throw ClipErr(CLIPGPU_ERR_INVALID, "host range not registered");
  });
}

int clipgpu_embed_tokens(clipgpu_engine* e, const int64_t* ids, const int64_t* mask, int64_t B, int64_t T,
                         float* out) {
  (void)mask;
  return guarded([&]() {
    need_tower(e, TOWER_TEXT);
    if (B <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
    if (!ids || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    if (T != e->spec.context_length)
      throw ClipErr(CLIPGPU_ERR_INVALID,
                    "Shape error: expected context length " + std::to_string(e->spec.context_length));
    for (int64_t i = 0; i < B * T; ++i)
      if (ids[i] < 0 || ids[i] >= e->spec.vocab_size)
        throw ClipErr(CLIPGPU_ERR_INVALID, "Inference error: token id " + std::to_string(ids[i]) + " out of range");
    // Sequence trimming: the pooled row of a sequence is its first argmax (EOT) token and
    // attention is causal, so tokens past the batch's last EOT never reach an embedding.
    // The batch runs on its first Tc = max(EOT index) + 1 tokens, rounded up to a multiple of 16,
    // bit-identical
    // (test_text_trim_is_bit_exact).  clipgpu_options.trim_text = -1 disables.  A trimmed batch is
    // a private copy, so it is staged even when `ids` lies in a registered range.
    int64_t Tc = T;
    // only for the causal, EOT-pooled (CLIP) form: SigLIP2's text tower attends to and pools
    // the last context position
    if (e->trim && e->spec.causal && !e->spec.pool_last) {
      Tc = 1;
      for (int64_t b = 0; b < B && Tc < T; ++b) {
        const int64_t* row = ids + b * T;
        int64_t best = 0;
        for (int64_t t = 1; t < T; ++t)
          if (row[t] > row[best]) best = t;
        Tc = std::max<int64_t>(Tc, best + 1);
      }
      // rounded up to a multiple of 16 (the causal key tiles are 16 wide, so any Tc past the
      // last EOT gives the same bits): at most ceil(T / 16) lengths reach the graph cache
      Tc = std::min<int64_t>(T, std::max<int64_t>((Tc + 15) / 16 * 16, 16));
    }
    std::vector<int64_t> trimmed;
    const int64_t* src = ids;
    if (Tc < T) {
      trimmed.resize((size_t)(B * Tc));
      for (int64_t b = 0; b < B; ++b) std::memcpy(&trimmed[(size_t)(b * Tc)], ids + b * T, (size_t)Tc * 8);
      src = trimmed.data();
    }
    std::lock_guard<std::mutex> lk(e->mu);
    run_host(*e, IN_IDS, HostRows{(const char*)src, nullptr, (size_t)Tc * 8}, B, nullptr, nullptr, out, (int)Tc);
  });
}

int clipgpu_embed_images_rgb8(clipgpu_engine* e, const uint8_t* const* images, const int* widths,
                              const int* heights, int64_t n, float* out) {
  return guarded([&]() {
    need_tower(e, TOWER_VISION);
    if (n <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");  // src/vision.rs:121-123
    if (!images || !widths || !heights || !out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    for (int64_t i = 0; i < n; ++i) {
      if (!images[i]) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL image");
      if (widths[i] <= 0 || heights[i] <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Resize error: empty image");
    }
    std::lock_guard<std::mutex> lk(e->mu);
    // A batch of S x S images needs no resize (the plan is the identity: a unit tap per output, exact) --
    // the images are the u8 NHWC rows, and the batch takes the u8 host path (copy pool staging in pieces,
    // copy-stream H2Ds, alternating buffer sets), bit-identical to the resize path
    // (test_embed_images_rgb8_identity_batches_take_the_u8_path).
    const int S = e->spec.image_size;
    bool identity = true;
    for (int64_t i = 0; i < n && identity; ++i) identity = widths[i] == S && heights[i] == S;
    if (identity) {
      const ResizePlan p = make_resize_plan(S, S, S, e->pre.interpolation, e->pre.resize_mode);
      identity = !p.need_h && !p.need_v;
    }
    if (identity && !e->rgb8_resize_always) {
      run_host(*e, IN_U8, HostRows{nullptr, (const void* const*)images, (size_t)3 * S * S}, n, e->pre.mean,
               e->pre.stdv, out);
      return;
    }
    run_sharded(*e, n, [&](Replica& r, int64_t b0, int64_t b1) {
      run_images_shard(*e, r, images, widths, heights, b0, b1, out);
    });
  });
}

int clipgpu_test_resize_rgb8_gpu(const uint8_t* const* images, const int* widths, const int* heights, int64_t n,
                                 int size, const char* interpolation, const char* resize_mode, uint8_t* out) {
  return guarded([&]() {
    if (n <= 0 || n > 65535 || size <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "bad resize batch");
    const ResizeBatch b = plan_resize_batch(size, interpolation ? interpolation : "bicubic",
                                            resize_mode ? resize_mode : "shortest", widths, heights, 0, (int)n);
    const size_t desc_bytes = align16(b.d.size() * sizeof(ResizeImage));
    const size_t ints_bytes = align16(b.ints.size() * sizeof(int));
    std::vector<char> host(desc_bytes + ints_bytes + b.raw_bytes);
    std::memcpy(host.data(), b.d.data(), b.d.size() * sizeof(ResizeImage));
    std::memcpy(host.data() + desc_bytes, b.ints.data(), b.ints.size() * sizeof(int));
    for (int64_t i = 0; i < n; ++i)
    {
      std::vector<CopyTask> tasks;
      add_window_tasks(tasks, b, (int)i, host.data() + desc_bytes + ints_bytes + b.raw_off[i], images[i], widths[i]);
      pool_copy(tasks);
    }
    char* dev = nullptr;
    uint8_t *tmp = nullptr, *dout = nullptr;
    const size_t out_bytes = (size_t)n * size * size * 3;
    HIP_CHECK(hipMalloc((void**)&dev, host.size()));
    HIP_CHECK(hipMalloc((void**)&tmp, std::max<size_t>(b.tmp_bytes, 16)));
    HIP_CHECK(hipMalloc((void**)&dout, out_bytes));
    HIP_CHECK(copy_h2d(dev, host.data(), host.size()));
    const hipError_t err = launch_resize((const uint8_t*)dev + desc_bytes + ints_bytes, tmp,
                                         (const int*)(dev + desc_bytes), (const ResizeImage*)dev, (int)n, b.max_th,
                                         size, dout, nullptr);
    const hipError_t err2 = copy_d2h(out, dout, out_bytes);
    (void)hipFree(dev);
    (void)hipFree(tmp);
    (void)hipFree(dout);
    check(err, "resize");
    check(err2, "resize copy-out");
  });
}

}  // extern "C"
