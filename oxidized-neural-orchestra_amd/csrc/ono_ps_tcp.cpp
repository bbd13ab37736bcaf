// ono_ps_tcp.cpp — parameter-server mode on the TCP edge: the server's
// per-worker task (parameter_server/src/service/pserver.rs:105-163) and the
// worker's ServerClusterManager (worker/src/middlewares/server_cluster.rs:7-105)
// over the caller's sockets, speaking the reference's frames byte for byte
// (comms/src/protocol/msg.rs:98-110, 160-191):
//   [u64 BE len = 4 + payload][u32 BE kind][payload]
//   1 / 2  DenseGrad  (is_last false / true): f16 LE values
//   3 / 4  SparseGrad (is_last false / true): the grad_drop stream
//   5      Params: f32 LE values
//   0 control (JSON), 6 data chunk, >= 7 invalid
// The ring's frame helpers (ono_tcp.cpp) take an ono_ring; this file has a
// small reader / writer of its own over the same header rules.  Every socket
// wait polls in 100 ms slices, watching an abort flag and a deadline.
//
// The server side is host logic around the store (ono_sync_step_f16 /
// ono_sync_step_sparse, where the device work is).  The worker side keeps the
// three buckets of every server in HBM and runs a push in stream order: per
// server the threshold into device memory, the stream-ordered drop (its length
// stays on the device) and the settle kernel that applies the compressor's
// size rule there (ono_kernels.hip PushSettleOp) — one host wait per
// push_grads, after which the host reads the lengths, frames and sends.
#include <hip/hip_runtime.h>

#include <poll.h>
#include <sys/socket.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <mutex>
#include <vector>

#include "ono_internal.h"

using namespace ono;

namespace {

constexpr int kPollMs = 100;  // abort latency
constexpr uint32_t KIND_DENSE = 1, KIND_DENSE_LAST = 2, KIND_SPARSE = 3, KIND_SPARSE_LAST = 4, KIND_PARAMS = 5,
                   KIND_MAX_VALID = 6;
constexpr size_t kSampleMax = 16384;             // SAMPLE_SIZE (protocol.rs:13-19)
constexpr size_t kZeroCopy = size_t(4) << 20;    // worst-case streams up to this are encoded into pinned frames
constexpr size_t kControlMax = size_t(16) << 20;  // a control frame longer than this is not parsed
constexpr double kDefaultTimeoutS = 600.0;

using Clock = std::chrono::steady_clock;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// One end of a connection: the socket, who may abort its waits, how long one wait may take.
struct Peer {
    int fd;
    const std::atomic<bool> *aborted;
    double timeout_s;
    const char *who;
};

Clock::time_point deadline_of(const Peer &p) {
    return Clock::now() + std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double>(p.timeout_s));
}

int wait_fd(const Peer &p, short ev, Clock::time_point deadline) {
    for (;;) {
        if (p.aborted->load()) return set_error(ONO_E_ABORTED, "aborted while waiting for the %s", p.who);
        const auto now = Clock::now();
        if (now >= deadline) return set_error(ONO_E_IO, "timed out after %g s waiting for the %s", p.timeout_s, p.who);
        const auto left = std::chrono::duration_cast<std::chrono::milliseconds>(deadline - now).count();
        struct pollfd pf = {p.fd, ev, 0};
        const int pr = poll(&pf, 1, (int)std::min<long long>(kPollMs, left + 1));
        if (pr < 0 && errno != EINTR) return set_error(ONO_E_IO, "poll: %s", strerror(errno));
        if (pr > 0) return ONO_OK;
    }
}

int send_all(const Peer &p, const uint8_t *buf, size_t n) {
    const auto deadline = deadline_of(p);
    size_t sent = 0;
    while (sent < n) {
        if (int rc = wait_fd(p, POLLOUT, deadline)) return rc;
        const ssize_t k = send(p.fd, buf + sent, n - sent, MSG_DONTWAIT | MSG_NOSIGNAL);
        if (k < 0 && errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR)
            return set_error(ONO_E_IO, "send to the %s: %s", p.who, strerror(errno));
        if (k > 0) sent += (size_t)k;
    }
    return ONO_OK;
}

int recv_all(const Peer &p, uint8_t *buf, size_t n, Clock::time_point deadline) {
    size_t got = 0;
    while (got < n) {
        if (int rc = wait_fd(p, POLLIN, deadline)) return rc;
        const ssize_t k = recv(p.fd, buf + got, n - got, MSG_DONTWAIT);
        if (k == 0) return set_error(ONO_E_IO, "the %s closed the connection", p.who);
        if (k < 0) {
            if (errno == EAGAIN || errno == EWOULDBLOCK || errno == EINTR) continue;
            return set_error(ONO_E_IO, "recv from the %s: %s", p.who, strerror(errno));
        }
        got += (size_t)k;
    }
    return ONO_OK;
}

// reads and drops n payload bytes (the connection stays framed)
int drain(const Peer &p, uint64_t n, Clock::time_point deadline) {
    uint8_t tmp[4096];
    while (n) {
        const size_t c = (size_t)std::min<uint64_t>(n, sizeof tmp);
        if (int rc = recv_all(p, tmp, c, deadline)) return rc;
        n -= c;
    }
    return ONO_OK;
}

void put_header(uint8_t *h, size_t payload, uint32_t kind) {
    const uint64_t flen = 4 + (uint64_t)payload;
    for (int i = 0; i < 8; i++) h[i] = (uint8_t)(flen >> (56 - 8 * i));
    for (int i = 0; i < 4; i++) h[8 + i] = (uint8_t)(kind >> (24 - 8 * i));
}

// The 12 header bytes of the next frame: its payload length and kind byte (msg.rs:98-110, 160-168, 187).
int recv_header(const Peer &p, uint64_t *payload, uint32_t *kind, Clock::time_point deadline) {
    uint8_t hdr[12];
    if (int rc = recv_all(p, hdr, 12, deadline)) return rc;
    uint64_t l = 0;
    for (int i = 0; i < 8; i++) l = (l << 8) | hdr[i];
    const uint32_t k = hdr[11];  // Header::from_be_bytes(..) as u8
    if (k > KIND_MAX_VALID) return set_error(ONO_E_IO, "Received an invalid kind byte %u", k);
    if (l < 4)
        return set_error(ONO_E_IO, "The given buffer is too small %llu, must at least be 4 bytes", (unsigned long long)l);
    *payload = l - 4;
    *kind = k;
    return ONO_OK;
}

// a pinned host buffer grown on demand, a quarter of headroom
struct Pinned {
    uint8_t *p = nullptr;
    size_t cap = 0;
    int grow(size_t need, unsigned flags = hipHostMallocDefault) {
        if (cap >= need) return ONO_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = need + need / 4;
        ONO_HIP(hipHostMalloc((void **)&p, want, flags));
        cap = want;
        return ONO_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

// ------------------------------------------------------------ server task ---
struct ono_server_task {
    ono_sync *sync = nullptr;
    ono_store *store = nullptr;
    int fd = -1;
    double timeout_s = kDefaultTimeoutS;
    std::atomic<bool> aborted{false};
    size_t nparams = 0;
    std::vector<uint8_t> frame;  // [4 pad][12 header][nparams f32]: the Params frame, stepped in place
    std::vector<uint8_t> rx;     // a received payload
};

extern "C" {

int ono_server_task_create(ono_server_task **out, ono_sync *sync, ono_store *store, int fd, double timeout_s) {
    if (!out) return set_error(ONO_E_ARG, "out is NULL");
    *out = nullptr;
    if (!sync || !store) return set_error(ONO_E_ARG, "NULL argument");
    if (fd < 0) return set_error(ONO_E_ARG, "fd %d", fd);
    if (int rc = ono_sync_clone(sync)) return rc;
    ono_server_task *t = new ono_server_task();
    t->sync = sync;
    t->store = store;
    t->fd = fd;
    t->timeout_s = timeout_s > 0 ? timeout_s : kDefaultTimeoutS;
    t->nparams = ono_store_len(store);
    t->frame.resize(16 + t->nparams * sizeof(float));
    *out = t;
    return ONO_OK;
}

int ono_server_task_run(ono_server_task *t) {
    if (!t) return set_error(ONO_E_ARG, "task is NULL");
    const Peer peer{t->fd, &t->aborted, t->timeout_s, "worker"};
    const size_t n = t->nparams;
    uint8_t *frame = t->frame.data() + 4;
    float *params = reinterpret_cast<float *>(t->frame.data() + 16);
    put_header(frame, n * sizeof(float), KIND_PARAMS);
    // pserver.rs:119-121
    if (int rc = ono_store_pull_params(t->store, n ? params : nullptr, n)) return rc;
    if (int rc = send_all(peer, frame, 12 + n * sizeof(float))) return rc;
    // the longest payload a gradient of n values can arrive in
    const uint64_t grad_max = std::max<uint64_t>(ono_sparse_max_bytes(n), 2 * (uint64_t)n);
    for (;;) {
        if (t->aborted.load()) return set_error(ONO_E_ABORTED, "server task aborted");
        const auto deadline = deadline_of(peer);
        uint64_t pay = 0;
        uint32_t kind = 0;
        if (int rc = recv_header(peer, &pay, &kind, deadline)) return rc;
        const bool dense = kind == KIND_DENSE || kind == KIND_DENSE_LAST;
        const bool sparse = kind == KIND_SPARSE || kind == KIND_SPARSE_LAST;
        const bool is_last = kind == KIND_DENSE_LAST || kind == KIND_SPARSE_LAST;
        if (!dense && !sparse) {  // pserver.rs:152-155 behind WorkerHandle::recv_event (handles/worker.rs:109-127)
            if (kind == 0 && pay <= kControlMax) {
                t->rx.resize((size_t)pay);
                if (int rc = recv_all(peer, t->rx.data(), (size_t)pay, deadline)) return rc;
                const int rc = ono_worker_event_check(kind, t->rx.data(), (size_t)pay);
                if (rc == ONO_E_IO && !strncmp(ono_last_error(), "loss diverged", 13)) return rc;
            }
            return set_error(ONO_E_PROTO, "invalid message");
        }
        if (dense) {
            if (pay % 2)  // bytemuck::cast_slice to f16 (msg.rs:175) cannot split a value
                return set_error(ONO_E_IO, "DenseGrad payload of %llu bytes is not a whole number of f16 values",
                                 (unsigned long long)pay);
            if (pay != 2 * (uint64_t)n) {  // :145-151: the reference warns and waits for the next frame
                if (int rc = drain(peer, pay, deadline)) return rc;
                continue;
            }
            t->rx.resize((size_t)pay);
            if (int rc = recv_all(peer, t->rx.data(), (size_t)pay, deadline)) return rc;
            if (int rc = ono_sync_step_f16(t->sync, t->store, reinterpret_cast<const uint16_t *>(t->rx.data()),
                                           n ? params : nullptr, n))
                return rc;
        } else {
            if (pay < 8) {
                if (int rc = drain(peer, pay, deadline)) return rc;
                return set_error(ONO_E_PROTO, "The given sparse buffer is smaller than TOTAL_LEN_SIZE");
            }
            uint8_t head[8];
            if (int rc = recv_all(peer, head, 8, deadline)) return rc;
            uint64_t total = 0;
            for (int q = 0; q < 8; q++) total |= (uint64_t)head[q] << (8 * q);
            if (total != n) {  // the gradient's length, read before the lift
                if (int rc = drain(peer, pay - 8, deadline)) return rc;
                continue;
            }
            if (pay > grad_max) {
                if (int rc = drain(peer, pay - 8, deadline)) return rc;
                return set_error(ONO_E_PROTO, "SparseGrad stream of %llu bytes for %zu values (at most %llu)",
                                 (unsigned long long)pay, n, (unsigned long long)grad_max);
            }
            t->rx.resize((size_t)pay);
            memcpy(t->rx.data(), head, 8);
            if (int rc = recv_all(peer, t->rx.data() + 8, (size_t)pay - 8, deadline)) return rc;
            if (int rc = ono_sync_step_sparse(t->sync, t->store, t->rx.data(), (size_t)pay, n ? params : nullptr, n))
                return rc;
        }
        if (is_last) return ONO_OK;  // :137-140
        if (t->aborted.load()) return set_error(ONO_E_ABORTED, "server task aborted");
        if (int rc = send_all(peer, frame, 12 + n * sizeof(float))) return rc;  // :142-143
    }
}

int ono_server_task_abort(ono_server_task *t) {
    if (!t) return set_error(ONO_E_ARG, "task is NULL");
    t->aborted.store(true);
    return ONO_OK;
}

int ono_server_task_destroy(ono_server_task *t) {
    if (!t) return ONO_OK;
    const int rc = ono_sync_release(t->sync);
    delete t;
    return rc;
}

}  // extern "C"

// ---------------------------------------------------------------- cluster ---
namespace {
struct Server {
    size_t size = 0, off = 0;  // values, and where the bucket starts in the flat allocations
    int fd = -1;
    uint64_t sample_state = 0;
    ono_sample_fn sampler = nullptr;
    void *sampler_ctx = nullptr;
    uint32_t *idx = nullptr, *idx_dev = nullptr;  // pinned: this push's threshold sample, read in place
    size_t sp_cap = 0;                            // ono_sparse_max_bytes(size)
    bool zc = false;                              // both encodings go straight into pinned frames
    // zc: [4 pad][12 header][stream] and [.. 12 header][f16 payload, phase-matched to the bucket]
    uint8_t *sp_frame = nullptr, *dn_frame = nullptr;
    // else: encoded in HBM, down into tx after the wait
    uint8_t *sp_dev = nullptr;
    uint16_t *dn_dev = nullptr;
    Pinned tx;
    // where this push's encodings land
    uint8_t *sp_buf = nullptr;
    uint16_t *out16 = nullptr;
};
}  // namespace

struct ono_cluster {
    int device = 0;
    double timeout_s = kDefaultTimeoutS;
    std::atomic<bool> aborted{false};
    std::mutex mu;  // one pull / push / acc at a time
    hipStream_t stream = nullptr;
    size_t total = 0;
    float *params = nullptr, *grad = nullptr, *residual = nullptr;
    std::vector<Server> sv;
    float ratio = 0.0f;
    float *t_dev = nullptr;        // per server: the push's threshold
    uint64_t *nb_dev = nullptr;    // per server: the drop stream's length
    uint64_t *nb_host = nullptr, *nb_host_dev = nullptr;  // the lengths, host-mapped, after the wait
    uint32_t *keys = nullptr;      // the threshold's scratch (kSampleMax words)
    uint64_t *word = nullptr, *word_dev = nullptr;  // the push's one wait
    uint32_t epoch = 0;
    hipEvent_t acc_ev = nullptr;
    bool acc_pending = false;
    Pinned rx;  // the Params payloads, server-major
};

namespace {

void cluster_free(ono_cluster *c) {
    DeviceGuard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (Server &s : c->sv) {
        if (s.idx) (void)hipHostFree(s.idx);
        if (s.sp_frame) (void)hipHostFree(s.sp_frame);
        if (s.dn_frame) (void)hipHostFree(s.dn_frame);
        (void)hipFree(s.sp_dev);
        (void)hipFree(s.dn_dev);
        s.tx.release();
    }
    for (void *p : {(void *)c->params, (void *)c->grad, (void *)c->residual, (void *)c->t_dev, (void *)c->nb_dev,
                    (void *)c->keys})
        (void)hipFree(p);
    if (c->nb_host) (void)hipHostFree(c->nb_host);
    if (c->word) (void)hipHostFree(c->word);
    c->rx.release();
    if (c->acc_ev) (void)hipEventDestroy(c->acc_ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int cluster_alloc(ono_cluster *c) {
    ONO_HIP(hipSetDevice(c->device));
    ONO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    ONO_HIP(hipEventCreateWithFlags(&c->acc_ev, hipEventDisableTiming));
    const size_t S = c->sv.size(), b = c->total * sizeof(float);
    for (float **p : {&c->params, &c->grad, &c->residual}) {
        ONO_HIP(hipMalloc((void **)p, b));
        ONO_HIP(hipMemset(*p, 0, b));
    }
    ONO_HIP(hipMalloc((void **)&c->t_dev, S * sizeof(float)));
    ONO_HIP(hipMalloc((void **)&c->nb_dev, S * sizeof(uint64_t)));
    ONO_HIP(hipMemset(c->t_dev, 0, S * sizeof(float)));
    ONO_HIP(hipMemset(c->nb_dev, 0, S * sizeof(uint64_t)));
    ONO_HIP(hipMalloc((void **)&c->keys, kSampleMax * sizeof(uint32_t)));
    ONO_HIP(hipHostMalloc((void **)&c->nb_host, S * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent));
    ONO_HIP(hipHostGetDevicePointer((void **)&c->nb_host_dev, c->nb_host, 0));
    ONO_HIP(hipHostMalloc((void **)&c->word, 2 * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent));
    ONO_HIP(hipHostGetDevicePointer((void **)&c->word_dev, c->word, 0));
    memset(c->nb_host, 0, S * sizeof(uint64_t));
    c->word[0] = c->word[1] = 0;
    if (int rc = c->rx.grow(b)) return rc;
    for (Server &s : c->sv) {
        ONO_HIP(hipHostMalloc((void **)&s.idx, kSampleMax * sizeof(uint32_t), hipHostMallocMapped));
        ONO_HIP(hipHostGetDevicePointer((void **)&s.idx_dev, s.idx, 0));
        s.sp_cap = ono_sparse_max_bytes(s.size);
        s.zc = s.sp_cap <= kZeroCopy;
        const size_t p = ph(s.off);  // the f16 payload shares the bucket's 4-element phase: the vector body runs
        if (s.zc) {
            ONO_HIP(hipHostMalloc((void **)&s.sp_frame, 16 + s.sp_cap + 64, hipHostMallocMapped | hipHostMallocCoherent));
            ONO_HIP(hipHostMalloc((void **)&s.dn_frame, 32 + 2 * (s.size + 4), hipHostMallocMapped | hipHostMallocCoherent));
            uint8_t *sp_d = nullptr, *dn_d = nullptr;
            ONO_HIP(hipHostGetDevicePointer((void **)&sp_d, s.sp_frame, 0));
            ONO_HIP(hipHostGetDevicePointer((void **)&dn_d, s.dn_frame, 0));
            s.sp_buf = sp_d + 16;
            s.out16 = reinterpret_cast<uint16_t *>(dn_d + 16) + p;
        } else {
            ONO_HIP(hipMalloc((void **)&s.sp_dev, s.sp_cap + 64));
            ONO_HIP(hipMalloc((void **)&s.dn_dev, 2 * (s.size + 4)));
            s.sp_buf = s.sp_dev;
            s.out16 = s.dn_dev + p;
            if (int rc = s.tx.grow(16 + 2 * s.size)) return rc;
        }
    }
    // the zero fills ran on the null stream, which the cluster's non-blocking stream is not ordered with
    ONO_HIP(hipStreamSynchronize(nullptr));
    return ONO_OK;
}

// the threshold sample of one push (as the ring's take_sample, without its look-ahead queue)
int draw_sample(Server &s, const uint32_t **idx_dev, size_t *m) {
    const size_t L = s.size;
    *m = std::min(L, kSampleMax);
    *idx_dev = nullptr;
    if (s.sampler) {  // called for every push, so a caller-side RNG stays in step with the reference's
        if (s.sampler(s.sampler_ctx, L, s.idx, *m) != 0)
            return set_error(ONO_E_OTHER, "the sampler failed for a gradient of %zu values", L);
        if (L <= kSampleMax) return ONO_OK;  // the gradient is its own sample
        for (size_t i = 0; i < *m; i++)
            if (s.idx[i] >= L) return set_error(ONO_E_ARG, "sample index %u out of %zu", s.idx[i], L);
    } else {
        if (L <= kSampleMax) return ONO_OK;
        if (int rc = ono_sparse_sample_default(&s.sample_state, L, s.idx, *m)) return rc;
    }
    *idx_dev = s.idx_dev;
    return ONO_OK;
}

int push_grads(ono_cluster *c, bool is_last) {
    hipStream_t st = c->stream;
    const size_t S = c->sv.size();
    const bool sparse_mode = c->ratio > 0.0f;
    if (c->acc_pending) {
        ONO_HIP(hipStreamWaitEvent(st, c->acc_ev, 0));
        c->acc_pending = false;
    }
    for (size_t j = 0; j < S; j++) {
        Server &s = c->sv[j];
        float *res = c->residual + s.off;
        if (!sparse_mode) {  // Base: f16(residual), residual = 0 (compressor.rs:106-118 + server_cluster.rs:90)
            ONO_HIP(launch_encode_zero<uint16_t>(s.out16, res, s.size, st));
            continue;
        }
        const uint32_t *idx_dev = nullptr;
        size_t m = 0;
        if (int rc = draw_sample(s, &idx_dev, &m)) return rc;
        if (int rc = sparse_threshold_dev(c->t_dev + j, res, s.size, idx_dev, c->keys, m, c->ratio, st)) return rc;
        if (int rc = sparse_drop_tdev_async(s.sp_buf, s.sp_cap, c->nb_dev + j, res, s.size, c->t_dev + j, st)) return rc;
        ONO_HIP(launch_push_settle(s.out16, res, s.size, c->t_dev + j, c->nb_dev + j, st));
    }
    if (sparse_mode)  // the S lengths to where the host reads them
        ONO_HIP(launch_copy<float>(reinterpret_cast<float *>(c->nb_host_dev), reinterpret_cast<const float *>(c->nb_dev),
                                   2 * S, st));
    if (++c->epoch == 0) c->epoch = 1;
    ONO_HIP(stream_wait(st, c->word, c->word_dev, c->epoch));  // the push's one wait
    if (sparse_mode)
        if (int rc = ono_sparse_drop_check(st)) return rc;
    // the frames: which encoding every server sends, and for the ones encoded in HBM its bytes down
    std::vector<const uint8_t *> frame(S);
    std::vector<size_t> bytes(S);
    bool staged = false;
    for (size_t j = 0; j < S; j++) {
        Server &s = c->sv[j];
        const uint64_t nb = sparse_mode ? c->nb_host[j] : 0;
        const bool sp = sparse_mode && nb <= 2 * (uint64_t)s.size;
        if (sparse_mode && (nb < 8 || nb > s.sp_cap))
            return set_error(ONO_E_IO, "sparse drop of server %zu reports a stream of %llu bytes", j, (unsigned long long)nb);
        const size_t pay = sp ? (size_t)nb : 2 * s.size;
        const uint32_t kind = sp ? (is_last ? KIND_SPARSE_LAST : KIND_SPARSE) : (is_last ? KIND_DENSE_LAST : KIND_DENSE);
        uint8_t *f;
        if (s.zc) {
            f = sp ? s.sp_frame + 4 : s.dn_frame + 4 + 2 * ph(s.off);
        } else {
            f = s.tx.p + 4;
            ONO_HIP(hipMemcpyAsync(f + 12, sp ? (const void *)s.sp_dev : (const void *)s.out16, pay, hipMemcpyDeviceToHost,
                                   st));
            staged = true;
        }
        put_header(f, pay, kind);
        frame[j] = f;
        bytes[j] = 12 + pay;
    }
    if (staged) ONO_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < S; j++) {
        const Peer peer{c->sv[j].fd, &c->aborted, c->timeout_s, "server"};
        if (int rc = send_all(peer, frame[j], bytes[j])) return rc;
    }
    return ONO_OK;
}

int pull_params(ono_cluster *c) {
    for (size_t j = 0; j < c->sv.size(); j++) {
        Server &s = c->sv[j];
        const Peer peer{s.fd, &c->aborted, c->timeout_s, "server"};
        const auto deadline = deadline_of(peer);
        uint64_t pay = 0;
        uint32_t kind = 0;
        if (int rc = recv_header(peer, &pay, &kind, deadline)) return rc;
        if (kind != KIND_PARAMS) {  // parameter_server.rs:75-78
            if (int rc = drain(peer, pay, deadline)) return rc;
            return set_error(ONO_E_IO, "Expected params from server %zu, got a frame of kind %u", j, kind);
        }
        if (pay != s.size * sizeof(float)) {
            if (int rc = drain(peer, pay, deadline)) return rc;
            return set_error(ONO_E_SIZE, "params of %llu bytes from server %zu, bucket of %zu values",
                             (unsigned long long)pay, j, s.size);
        }
        uint8_t *dst = c->rx.p + s.off * sizeof(float);
        if (int rc = recv_all(peer, dst, (size_t)pay, deadline)) return rc;
        ONO_HIP(hipMemcpyAsync(c->params + s.off, dst, (size_t)pay, hipMemcpyHostToDevice, c->stream));
    }
    ONO_HIP(hipStreamSynchronize(c->stream));
    return ONO_OK;
}

}  // namespace

extern "C" {

int ono_cluster_create(ono_cluster **out, int nservers, const size_t *sizes, const int *fds, int device,
                       double timeout_s) {
    if (!out) return set_error(ONO_E_ARG, "out is NULL");
    *out = nullptr;
    if (nservers < 1 || !sizes || !fds) return set_error(ONO_E_ARG, "nservers=%d", nservers);
    ono_cluster *c = new ono_cluster();
    c->device = device;
    c->timeout_s = timeout_s > 0 ? timeout_s : kDefaultTimeoutS;
    c->sv.resize((size_t)nservers);
    for (int j = 0; j < nservers; j++) {
        if (sizes[j] < 1 || sizes[j] >= 0xFFFFFFFFull || fds[j] < 0) {
            delete c;
            return set_error(ONO_E_ARG, "server %d: %zu parameters, fd %d", j, sizes[j], fds[j]);
        }
        c->sv[j].size = sizes[j];
        c->sv[j].off = c->total;
        c->sv[j].fd = fds[j];
        c->total += sizes[j];
    }
    DeviceGuard g(device);
    if (int rc = cluster_alloc(c)) {
        cluster_free(c);
        return rc;
    }
    *out = c;
    return ONO_OK;
}

int ono_cluster_set_sparse(ono_cluster *c, float ratio, uint64_t seed) {
    if (!c) return set_error(ONO_E_ARG, "cluster is NULL");
    if (!(ratio == 0.0f || (ratio > 0.0f && ratio <= 1.0f)))
        return set_error(ONO_E_ARG, "ratio %g: SparseCapable keeps a fraction in (0, 1], 0 = the Base serializer",
                         (double)ratio);
    std::lock_guard<std::mutex> lk(c->mu);
    c->ratio = ratio;
    for (Server &s : c->sv) s.sample_state = seed;
    return ONO_OK;
}

int ono_cluster_set_sampler(ono_cluster *c, int server, ono_sample_fn fn, void *ctx) {
    if (!c || server < 0 || (size_t)server >= c->sv.size()) return set_error(ONO_E_ARG, "server %d", server);
    std::lock_guard<std::mutex> lk(c->mu);
    c->sv[server].sampler = fn;
    c->sv[server].sampler_ctx = ctx;
    return ONO_OK;
}

static float *bucket(ono_cluster *c, int server, float *base) {
    if (!c || server < 0 || (size_t)server >= c->sv.size()) return nullptr;
    return base + c->sv[server].off;
}
float *ono_cluster_params(ono_cluster *c, int server) { return bucket(c, server, c ? c->params : nullptr); }
float *ono_cluster_grad(ono_cluster *c, int server) { return bucket(c, server, c ? c->grad : nullptr); }
float *ono_cluster_residual(ono_cluster *c, int server) { return bucket(c, server, c ? c->residual : nullptr); }
size_t ono_cluster_size(const ono_cluster *c, int server) {
    return (!c || server < 0 || (size_t)server >= c->sv.size()) ? 0 : c->sv[server].size;
}

int ono_cluster_pull_params(ono_cluster *c) {
    if (!c) return set_error(ONO_E_ARG, "cluster is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return pull_params(c);
}

int ono_cluster_acc_residual(ono_cluster *c, void *stream) {
    if (!c) return set_error(ONO_E_ARG, "cluster is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ONO_HIP(launch_acc(c->residual, c->grad, c->total, s, true));
    ONO_HIP(hipEventRecord(c->acc_ev, s));
    c->acc_pending = true;
    return ONO_OK;
}

int ono_cluster_push_grads(ono_cluster *c, int is_last) {
    if (!c) return set_error(ONO_E_ARG, "cluster is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->aborted.load()) return set_error(ONO_E_ABORTED, "cluster aborted");
    DeviceGuard g(c->device);
    return push_grads(c, is_last != 0);
}

int ono_cluster_abort(ono_cluster *c) {
    if (!c) return set_error(ONO_E_ARG, "cluster is NULL");
    c->aborted.store(true);
    return ONO_OK;
}

int ono_cluster_destroy(ono_cluster *c) {
    if (!c) return ONO_OK;
    cluster_free(c);
    return ONO_OK;
}

}  // extern "C"
