// dist_rccl.cpp -- the built-in transport of the exchange plan (dist.hpp, include/sparsex_hip.h):
// RCCL point-to-point over xGMI, librccl loaded on demand.  xGMI is point-to-point: every pair of
// GPUs has its own link, so the direct pairwise exchange is the collective that fits it -- a ring
// would push every byte over up to seven links.
#include "dist.hpp"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace spx {

namespace {

struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;      // (optional)
};

Rccl &rccl()
{
    static Rccl r;
    if (r.lib) return r;
    // loaded on demand: a single-GPU user of this library never maps librccl
    // (a copy the process has mapped already -- e.g. the one PyTorch ships -- is
    // taken first, so that there is one RCCL per process)
    for (int flags : {RTLD_NOW | RTLD_NOLOAD, RTLD_NOW | RTLD_GLOBAL}) {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, flags);
            if (r.lib) break;
        }
        if (r.lib) break;
    }
    if (!r.lib) throw FatalError(std::string("cannot load librccl: ") + dlerror());
#define SPX_SYM(field, sym)                                                                      \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, sym));                            \
    if (!r.field) throw FatalError(std::string("librccl lacks ") + sym)
    SPX_SYM(GetUniqueId, "ncclGetUniqueId");
    SPX_SYM(CommInitRank, "ncclCommInitRank");
    SPX_SYM(CommDestroy, "ncclCommDestroy");
    SPX_SYM(GroupStart, "ncclGroupStart");
    SPX_SYM(GroupEnd, "ncclGroupEnd");
    SPX_SYM(Send, "ncclSend");
    SPX_SYM(Recv, "ncclRecv");
    SPX_SYM(GetErrorString, "ncclGetErrorString");
    r.CommCount = reinterpret_cast<decltype(r.CommCount)>(dlsym(r.lib, "ncclCommCount"));
#undef SPX_SYM
    return r;
}

struct RcclCtx {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    hipStream_t setup_stream = nullptr;
    // set-up exchanges: a status word per peer (allocated with the communicator, so that a
    // rank can always say that something went wrong on its side) and the staging buffers
    double *st_send = nullptr, *st_recv = nullptr;       // `world` doubles each
    double *stage_s = nullptr, *stage_r = nullptr;
    size_t cap_s = 0, cap_r = 0;
};

int rccl_exchange_device(void *ctx_, const double *send, const size_t *soff, const size_t *scnt,
                         double *recv, const size_t *roff, const size_t *rcnt, void *stream)
{
    RcclCtx *c = static_cast<RcclCtx *>(ctx_);
    Rccl &r = rccl();
    hipStream_t st = static_cast<hipStream_t>(stream);
    ncclResult_t rc = r.GroupStart();
    for (int q = 0; q < c->world && rc == ncclSuccess; ++q) {
        if (q == c->rank) continue;
        if (scnt[q]) rc = r.Send(send + soff[q], scnt[q], ncclDouble, q, c->comm, st);
        if (rc == ncclSuccess && rcnt[q]) rc = r.Recv(recv + roff[q], rcnt[q], ncclDouble, q, c->comm, st);
    }
    const ncclResult_t rc2 = r.GroupEnd();
    if (rc == ncclSuccess) rc = rc2;
    if (rc != ncclSuccess) {
        log_msg(LOG_ERR, "RCCL: %s\n", r.GetErrorString(rc));
        return -1;
    }
    return 0;
}

static bool grow(double *&buf, size_t &cap, size_t want)
{
    if (want <= cap) return true;
    if (buf) (void) hipFree(buf);
    buf = nullptr;
    cap = 0;
    if (hipMalloc(reinterpret_cast<void **>(&buf), want * 8) != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    cap = want;
    return true;
}

int rccl_exchange_host(void *ctx_, const uint64_t *send, const size_t *soff, const size_t *scnt,
                       uint64_t *recv, const size_t *roff, const size_t *rcnt)
{
    // set-up time only: staged through device buffers (8-byte words travel as doubles,
    // nothing looks at the bits).  Whatever can fail locally -- growing the staging
    // buffers, the upload -- happens BEFORE the group, and its outcome travels first, as a
    // status word per peer through buffers that exist since the communicator was made: a
    // rank that cannot take part in the payload exchange says so, and every rank returns
    // -1 together instead of waiting for it inside ncclRecv.
    RcclCtx *c = static_cast<RcclCtx *>(ctx_);
    const size_t W = (size_t) c->world;
    size_t ns = 0, nr = 0;
    for (int q = 0; q < c->world; ++q) {
        if (q == c->rank) continue;
        ns = std::max(ns, soff[q] + scnt[q]);
        nr = std::max(nr, roff[q] + rcnt[q]);
    }
    bool ok = grow(c->stage_s, c->cap_s, std::max<size_t>(ns, 1)) && grow(c->stage_r, c->cap_r, std::max<size_t>(nr, 1));
    if (ok && ns && hipMemcpyAsync(c->stage_s, send, ns * 8, hipMemcpyHostToDevice, c->setup_stream) != hipSuccess) {
        (void) hipGetLastError();
        ok = false;
    }
    // the status round: one word to and from every peer
    std::vector<double> st(W, ok ? 0.0 : 1.0), got(W, 0.0);
    std::vector<size_t> off(W), one(W, 1);
    for (size_t q = 0; q < W; ++q) off[q] = q;
    one[(size_t) c->rank] = 0;
    // (the status words go up with a synchronous copy; should even that fail, this rank STILL enters
    // the group -- with whatever the buffer held last -- because a rank that stays away leaves its
    // peers waiting inside ncclRecv, and RCCL has no timeout: it then fails locally, and the peers
    // are bounded by their caller's watchdog, bench.py's Watchdog for one)
    const bool staged = hipMemcpy(c->st_send, st.data(), W * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (!staged) (void) hipGetLastError();
    if (rccl_exchange_device(c, c->st_send, off.data(), one.data(), c->st_recv, off.data(), one.data(),
                             c->setup_stream) != 0 ||
        hipMemcpyAsync(got.data(), c->st_recv, W * 8, hipMemcpyDeviceToHost, c->setup_stream) != hipSuccess ||
        hipStreamSynchronize(c->setup_stream) != hipSuccess || !staged) {
        (void) hipGetLastError();
        log_msg(LOG_ERR, "RCCL transport: the status round of a set-up exchange failed\n");
        return -1;
    }
    for (size_t q = 0; q < W; ++q)
        if (q != (size_t) c->rank && got[q] != 0.0) ok = false;
    if (!ok) {
        log_msg(LOG_ERR, "RCCL transport: a rank could not stage its set-up exchange; all ranks give up\n");
        return -1;
    }
    if (rccl_exchange_device(c, c->stage_s, soff, scnt, c->stage_r, roff, rcnt, c->setup_stream) != 0 ||
        hipStreamSynchronize(c->setup_stream) != hipSuccess)
        return -1;
    // only the segments that were received are defined
    for (int q = 0; q < c->world; ++q)
        if (q != c->rank && rcnt[q] &&
            hipMemcpy(recv + roff[q], c->stage_r + roff[q], rcnt[q] * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return -1;
    return 0;
}

}  // namespace

}  // namespace spx

extern "C" {

spx_error_t spx_hip_rccl_unique_id(void *id)
{
    static_assert(sizeof(ncclUniqueId) == SPX_RCCL_ID_BYTES, "RCCL id size");
    try {
        ncclUniqueId u;
        if (!id || spx::rccl().GetUniqueId(&u) != ncclSuccess) return SPX_FAILURE;
        memcpy(id, &u, sizeof(u));
    } catch (const spx::FatalError &e) {
        spx::log_msg(spx::LOG_ERR, "%s\n", e.what.c_str());
        return SPX_FAILURE;
    }
    return SPX_SUCCESS;
}

spx_hip_transport_t *spx_hip_transport_rccl(const void *id, int rank, int world)
{
    if (!id || world < 1 || rank < 0 || rank >= world) return NULL;
    try {
        spx::Rccl &r = spx::rccl();
        std::unique_ptr<spx::RcclCtx> c(new spx::RcclCtx);
        c->rank = rank;
        c->world = world;
        ncclUniqueId u;
        memcpy(&u, id, sizeof(u));
        const ncclResult_t rc = r.CommInitRank(&c->comm, world, u, rank);
        if (rc != ncclSuccess) {
            spx::log_msg(spx::LOG_ERR, "RCCL communicator: %s\n", r.GetErrorString(rc));
            return NULL;
        }
        if (hipStreamCreateWithFlags(&c->setup_stream, hipStreamNonBlocking) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&c->st_send), (size_t) world * 8) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&c->st_recv), (size_t) world * 8) != hipSuccess) {
            // (the communicator exists on the other ranks and destroying it here does not reach them:
            // a peer that goes on to its first exchange waits until its caller's watchdog ends it)
            (void) r.CommDestroy(c->comm);
            if (c->setup_stream) (void) hipStreamDestroy(c->setup_stream);
            (void) hipFree(c->st_send);
            (void) hipFree(c->st_recv);
            (void) hipGetLastError();
            return NULL;
        }
        spx_hip_transport_t *t = new spx_hip_transport_t;
        t->ctx = c.release();
        t->rank = rank;
        t->world = world;
        t->exchange_host = spx::rccl_exchange_host;
        t->exchange_device = spx::rccl_exchange_device;
        return t;
    } catch (const spx::FatalError &e) {
        spx::log_msg(spx::LOG_ERR, "%s\n", e.what.c_str());
        return NULL;
    }
}

int spx_hip_transport_rccl_ranks(const spx_hip_transport_t *t)
{
    if (!t || t->exchange_device != spx::rccl_exchange_device || !t->ctx) return -1;
    try {
        spx::Rccl &r = spx::rccl();
        const spx::RcclCtx *c = static_cast<const spx::RcclCtx *>(t->ctx);
        int n = -1;
        if (!r.CommCount || !c->comm || r.CommCount(c->comm, &n) != ncclSuccess) return -1;
        return n;
    } catch (...) {
        return -1;
    }
}

void spx_hip_transport_destroy(spx_hip_transport_t *t)
{
    // (only transports made by spx_hip_transport_rccl)
    if (!t) return;
    spx::RcclCtx *c = static_cast<spx::RcclCtx *>(t->ctx);
    if (c) {
        if (c->comm) (void) spx::rccl().CommDestroy(c->comm);
        if (c->setup_stream) (void) hipStreamDestroy(c->setup_stream);
        (void) hipFree(c->st_send); (void) hipFree(c->st_recv);
        (void) hipFree(c->stage_s); (void) hipFree(c->stage_r);
        delete c;
    }
    delete t;
}

}  // extern "C"
