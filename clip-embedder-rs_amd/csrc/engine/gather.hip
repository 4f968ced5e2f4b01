// The handle's RCCL communicators and the gathered entry points.
#include "engine.hpp"

namespace clipgpu {

#define NCCL_CHECK(expr)                                                                            \
  do {                                                                                              \
    ncclResult_t _r = (expr);                                                                       \
    if (_r != ncclSuccess)                                                                          \
      throw ClipErr(CLIPGPU_ERR_DEVICE, std::string("RCCL error: ") + ncclGetErrorString(_r) + " (" #expr ")"); \
  } while (0)

// ---- sharded forward + the RCCL all-gather of the embedding rows ----------
// Every rank embeds its own contiguous block of rows[rank] rows into its slot of a [sum rows][E]
// output on its device, then one collective leaves the whole matrix, in rank order, on every
// rank: an in-place ncclAllGather when all blocks are equal, else (ragged blocks) one in-place
// ncclBroadcast per non-empty block inside a group.  `local` is replica i = rank rank0 + i.
// The multi-device handle's communicator, created on its first gathered call (clipgpu_create_ex).
void ensure_comm(clipgpu_engine& e) {
  if (!e.comm_pending) return;
  std::vector<ncclComm_t> comms(e.comm_devs.size());
  NCCL_CHECK(ncclCommInitAll(comms.data(), (int)comms.size(), e.comm_devs.data()));
  for (size_t i = 0; i < comms.size(); ++i) e.reps[i].comm = comms[i];
  e.comm_pending = false;
}

namespace {

// Host-side plan of a gathered call (no GPU; clipgpu_test_gather_plan checks it on the CPU):
// off[r] = first output row of rank r's block (rank order), equal = every block the same size
// (one ncclAllGather; else one ncclBroadcast per non-empty block), and per local replica the
// forward chunks of at most max_batch rows, each written at its rows of the output.
struct GatherPlan {
  std::vector<int64_t> off;
  bool equal = true;
};
GatherPlan plan_gather(int nr, const int64_t* rows) {
  GatherPlan g;
  g.off.assign((size_t)nr + 1, 0);
  for (int r = 0; r < nr; ++r) {
    if (rows[r] < 0) throw ClipErr(CLIPGPU_ERR_INVALID, "negative row count");
    g.off[r + 1] = g.off[r] + rows[r];
    g.equal = g.equal && rows[r] == rows[0];
  }
  if (g.off[nr] == 0) throw ClipErr(CLIPGPU_ERR_INVALID, "Empty batch");
  return g;
}

template <typename Fwd>
void sharded_gather(clipgpu_engine& e, const int64_t* rows, float* const* d_out, void* const* streams, Fwd fwd) {
  const int nr = e.comm_nranks, E = e.spec.embed_dim, G = (int)e.reps.size();
  if (nr <= 0) throw ClipErr(CLIPGPU_ERR_INVALID, "no communicator: create the handle over distinct devices "
                                                  "or call clipgpu_comm_init_rank first");
  const GatherPlan plan = plan_gather(nr, rows);
  const std::vector<int64_t>& off = plan.off;
  // (test hook clipgpu_test_force_broadcast: the ragged branch with equal blocks)
  const bool equal = plan.equal && !e.force_bcast;
  std::vector<hipStream_t> sts((size_t)G);
  for (int i = 0; i < G; ++i) {
    Replica& r = e.reps[i];
    if (!d_out[i]) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    // NULL array / entry: the legacy default stream of the replica's device, as in the single-device
    // entry points (run_graph forks the forward from it and joins it back; the collective runs on it)
    sts[i] = streams ? (hipStream_t)streams[i] : nullptr;
    const int rank = e.comm_rank0 + i;
    HIP_CHECK(hipSetDevice(r.device));
    for (int64_t c0 = 0; c0 < rows[rank]; c0 += e.max_batch)
      fwd(r, i, c0, (int)std::min<int64_t>(e.max_batch, rows[rank] - c0), d_out[i] + (off[rank] + c0) * E, sts[i]);
  }
  ensure_comm(e);
  NCCL_CHECK(ncclGroupStart());
  for (int i = 0; i < G; ++i) {
    Replica& r = e.reps[i];
    const int rank = e.comm_rank0 + i;
    if (equal) {
      NCCL_CHECK(ncclAllGather(d_out[i] + off[rank] * E, d_out[i], (size_t)rows[rank] * E, ncclFloat, r.comm, sts[i]));
    } else {
      for (int q = 0; q < nr; ++q)
        if (rows[q] > 0)
          NCCL_CHECK(ncclBroadcast(d_out[i] + off[q] * E, d_out[i] + off[q] * E, (size_t)rows[q] * E, ncclFloat, q,
                                   r.comm, sts[i]));
    }
  }
  NCCL_CHECK(ncclGroupEnd());
  // destroy_comms waits for these (the collective runs on the caller's stream, not the handle's)
  for (int i = 0; i < G; ++i) {
    Replica& r = e.reps[i];
    HIP_CHECK(hipSetDevice(r.device));
    if (!r.coll) HIP_CHECK(hipEventCreateWithFlags(&r.coll, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(r.coll, sts[i]));
  }
}

}  // namespace

// The handle's communicators: collectives may still be in flight on callers' streams, so each
// replica's last collective (the event recorded behind it on the caller's stream) and the handle's own
// streams are waited for first -- not the whole device, which may run unrelated work (torch, other
// engines); then all of the clique's communicators are finalized inside one group (a one-by-one
// finalize from one thread can block on peers) and destroyed.
void destroy_comms(clipgpu_engine& e) {
  bool any = false;
  for (auto& r : e.reps)
    if (r.comm) {
      (void)hipSetDevice(r.device);
      if (r.coll) (void)hipEventSynchronize(r.coll);
      if (r.stream) (void)hipStreamSynchronize(r.stream);
      for (int i = 0; i < 4; ++i)
        if (r.lane[i]) (void)hipStreamSynchronize(r.lane[i]);
      any = true;
    }
  if (!any) return;
  if (ncclGroupStart() == ncclSuccess) {
    for (auto& r : e.reps)
      if (r.comm) (void)ncclCommFinalize(r.comm);
    (void)ncclGroupEnd();
  }
  for (auto& r : e.reps)
    if (r.comm) {
      (void)ncclCommDestroy(r.comm);
      r.comm = nullptr;
    }
}

}  // namespace clipgpu

using namespace clipgpu;

extern "C" {

int clipgpu_comm_unique_id(uint8_t* id) {
  return guarded([&]() {
    if (!id) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL id");
    ncclUniqueId u;
    NCCL_CHECK(ncclGetUniqueId(&u));
    std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  });
}

int clipgpu_comm_init_rank(clipgpu_engine* e, const uint8_t* id, int nranks, int rank) {
  return guarded([&]() {
    if (!e || !id) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    if (e->reps.size() != 1) throw ClipErr(CLIPGPU_ERR_INVALID, "clipgpu_comm_init_rank needs a one-device handle");
    if (nranks < 1 || rank < 0 || rank >= nranks) throw ClipErr(CLIPGPU_ERR_INVALID, "bad nranks / rank");
    std::lock_guard<std::mutex> lk(e->mu);
    Replica& r = e->reps[0];
    if (r.comm) throw ClipErr(CLIPGPU_ERR_INVALID, "the handle already has a communicator");
    ncclUniqueId u;
    std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    HIP_CHECK(hipSetDevice(r.device));
    NCCL_CHECK(ncclCommInitRank(&r.comm, nranks, u, rank));
    e->comm_nranks = nranks;
    e->comm_rank0 = rank;
  });
}

int clipgpu_comm_info(const clipgpu_engine* e, int* nranks, int* rank0) {
  return guarded([&]() {
    if (!e || !nranks || !rank0) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL argument");
    *nranks = e->comm_nranks;
    *rank0 = e->comm_rank0;
  });
}

int clipgpu_embed_pixels_gather_device(clipgpu_engine* e, const float* const* d_nchw, const int64_t* rows,
                                       float* const* d_out, void* const* streams) {
  return guarded([&]() {
    need_tower(e, TOWER_VISION);
    if (!d_nchw || !rows || !d_out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t row_bytes = (size_t)3 * e->spec.image_size * e->spec.image_size * 4;
    sharded_gather(*e, rows, d_out, streams, [&](Replica& r, int i, int64_t c0, int n, float* dst, hipStream_t st) {
      if (!d_nchw[i]) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
      const float* src = (const float*)((const char*)d_nchw[i] + c0 * row_bytes);
      run_graph(*e, r, {1, (uint64_t)src, (uint64_t)dst, (uint64_t)n}, st, [&](hipStream_t gs) {
        vision_forward_lanes(*e, r, src, A_IMG_F32, nullptr, nullptr, n, dst, gs);
      });
    });
  });
}

int clipgpu_embed_tokens_gather_device(clipgpu_engine* e, const int64_t* const* d_ids, const int64_t* rows,
                                       float* const* d_out, void* const* streams) {
  return guarded([&]() {
    need_tower(e, TOWER_TEXT);
    if (!d_ids || !rows || !d_out) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(e->mu);
    const int T = e->spec.context_length;
    sharded_gather(*e, rows, d_out, streams, [&](Replica& r, int i, int64_t c0, int n, float* dst, hipStream_t st) {
      if (!d_ids[i]) throw ClipErr(CLIPGPU_ERR_INVALID, "NULL buffer");
      const int64_t* src = d_ids[i] + c0 * T;
      run_graph(*e, r, {3, (uint64_t)src, (uint64_t)dst, (uint64_t)n}, st,
                [&](hipStream_t gs) { text_forward_lanes(*e, r, src, n, dst, gs); });
    });
  });
}

int clipgpu_test_gather_plan(int nranks, const int64_t* rows, int64_t* off, int* equal) {
  return guarded([&]() {
    if (nranks < 1 || !rows || !off || !equal) throw ClipErr(CLIPGPU_ERR_INVALID, "bad arguments");
    const GatherPlan g = plan_gather(nranks, rows);
    for (int r = 0; r <= nranks; ++r) off[r] = g.off[r];
    *equal = g.equal ? 1 : 0;
  });
}

}  // extern "C"
