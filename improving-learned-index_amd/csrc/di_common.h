// di_common.h -- shared host-side plumbing of libdeepimpact_hip.so:
// error reporting across the C ABI, HIP checks, device buffers, per-kernel
// HIP-event timing, and what every entry point does with its arguments (device
// scope, staging in and out, small read-backs, offset checks).  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <initializer_list>
#include <map>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/deepimpact.h"

namespace di {

// thread-local last error (di_last_error)
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *last_error();
int n_cu();  // compute units of the current device

struct Error {
    int code;
};

// Host worker threads of the library's host-side passes (index build, synthetic
// collections): DI_HOST_THREADS, else OMP_NUM_THREADS (16 on the GPU box), else the
// hardware count; at most 64.
inline int host_threads() {
    const char *e = std::getenv("DI_HOST_THREADS");
    if (!e) e = std::getenv("OMP_NUM_THREADS");
    const int t = e ? std::atoi(e) : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(t > 0 ? t : 1, 64));
}

// f(lo, hi, thread) over [0, n) split in `threads` contiguous ranges (thread t always
// gets the same range for the same n and threads).  A worker's exception -- a
// di::Error with its thread-local message, std::bad_alloc, anything -- is carried to
// the calling thread and rethrown there after every worker has joined (the lowest
// thread's), so the C-ABI guard turns it into a status code instead of
// std::terminate.
template <class F>
void parallel_for_threads(int64_t n, int threads, F &&f) {
    const int T = (int)std::min<int64_t>(std::max(threads, 1), std::max<int64_t>(n, 1));
    if (T == 1) {
        f((int64_t)0, n, 0);
        return;
    }
    std::vector<std::exception_ptr> err((size_t)T);
    std::vector<int> code((size_t)T, 0);
    std::vector<std::string> msg((size_t)T);
    std::vector<std::thread> th;
    th.reserve((size_t)T);
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            try {
                f(n * t / T, n * (t + 1) / T, t);
            } catch (const Error &e) {
                code[(size_t)t] = e.code;
                msg[(size_t)t] = last_error();
                err[(size_t)t] = std::current_exception();
            } catch (...) {
                err[(size_t)t] = std::current_exception();
            }
        });
    for (auto &x : th) x.join();
    for (int t = 0; t < T; ++t)
        if (err[(size_t)t]) {
            if (code[(size_t)t]) {
                set_error("%s", msg[(size_t)t].c_str());
                throw Error{code[(size_t)t]};
            }
            std::rethrow_exception(err[(size_t)t]);
        }
}

template <class F>
void parallel_for(int64_t n, F &&f) {
    parallel_for_threads(n, host_threads(), std::forward<F>(f));
}

// parallel_for over n chunks whose bodies may throw di::Error: f(chunk, thread).  The
// lowest-index failing chunk's error (code and message -- di_last_error is thread-local)
// is rethrown on the calling thread, the one a serial loop would have raised first.
template <class F>
void parallel_chunks(int64_t n, F &&f) {
    std::vector<int> code((size_t)std::max<int64_t>(n, 1), 0);
    std::vector<std::string> msg((size_t)std::max<int64_t>(n, 1));
    parallel_for(n, [&](int64_t lo, int64_t hi, int t) {
        for (int64_t c = lo; c < hi; ++c) {
            try {
                f(c, t);
            } catch (const Error &e) {
                code[(size_t)c] = e.code;
                msg[(size_t)c] = last_error();
                return;  // (later chunks of this thread come after the failure)
            } catch (...) {
                code[(size_t)c] = DI_ENOMEM;
                msg[(size_t)c] = "host allocation failed";
                return;
            }
        }
    });
    for (int64_t c = 0; c < n; ++c)
        if (code[(size_t)c]) {
            set_error("%s", msg[(size_t)c].c_str());
            throw Error{code[(size_t)c]};
        }
}

// body(); a di::Error it throws gets "line N: " in front of its message, N = line_of()
// (1-based; evaluated on the error path only, so it may rescan the input).
template <class Body, class LineOf>
void with_line_context(Body &&body, LineOf &&line_of) {
    try {
        body();
    } catch (const Error &) {
        const std::string m = last_error();
        set_error("line %lld: %s", (long long)line_of(), m.c_str());
        throw;
    }
}

[[noreturn]] inline void fail(int code, const char *msg) {
    set_error("%s", msg);
    throw Error{code};
}

#define DI_HIP(expr)                                                                    \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ::di::set_error("%s:%d %s: %s", __FILE__, __LINE__, #expr,                  \
                            hipGetErrorString(e_));                                     \
            throw ::di::Error{e_ == hipErrorOutOfMemory ? DI_ENOMEM : DI_EHIP};         \
        }                                                                               \
    } while (0)

#define DI_REQUIRE(cond, code, ...)                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            ::di::set_error(__VA_ARGS__);                                               \
            throw ::di::Error{code};                                                    \
        }                                                                               \
    } while (0)

// Run a C-ABI body, translating exceptions into status codes.
template <class F>
int guard(F &&f) {
    try {
        f();
        return DI_OK;
    } catch (const Error &e) {
        return e.code;
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return DI_ENOMEM;
    } catch (...) {
        set_error("unexpected C++ exception");
        return DI_EINVAL;
    }
}

// Owning device buffer (grows, never shrinks).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    void reserve(size_t n) {
        if (n <= bytes) return;
        if (p) DI_HIP(hipFree(p));
        p = nullptr;
        bytes = 0;
        DI_HIP(hipMalloc(&p, n ? n : 16));
        bytes = n;
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

// Per-kernel timing with HIP events recorded on the launching stream.
struct Timer {
    struct Pending {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::map<std::string, std::pair<double, int64_t>> acc;
    std::vector<hipEvent_t> pool;

    hipEvent_t ev() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        DI_HIP(hipEventCreate(&e));
        return e;
    }
    void begin(bool on, const char *name, hipStream_t s, hipEvent_t *a) {
        if (!on) return;
        *a = ev();
        DI_HIP(hipEventRecord(*a, s));
        pending.push_back({name, *a, nullptr});
    }
    void end(bool on, hipStream_t s) {
        if (!on) return;
        hipEvent_t b = ev();
        DI_HIP(hipEventRecord(b, s));
        pending.back().b = b;
    }
    // call after the stream has been synchronised
    void resolve() {
        for (auto &p : pending) {
            float ms = 0.f;
            DI_HIP(hipEventElapsedTime(&ms, p.a, p.b));
            auto &e = acc[p.name];
            e.first += ms;
            e.second += 1;
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
    void get(const char *name, di_timing *out, bool reset) {
        auto it = acc.find(name);
        out->ms = it == acc.end() ? 0.0 : it->second.first;
        out->launches = it == acc.end() ? 0 : it->second.second;
        if (reset) acc.clear();
    }
    ~Timer() {
        for (auto &p : pending) {
            (void)hipEventDestroy(p.a);
            if (p.b) (void)hipEventDestroy(p.b);
        }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

// RAII timing scope around one kernel launch.
struct TimedLaunch {
    Timer &t;
    bool on;
    hipStream_t s;
    TimedLaunch(Timer &t_, bool on_, const char *name, hipStream_t s_) : t(t_), on(on_), s(s_) {
        hipEvent_t a;
        t.begin(on, name, s, &a);
    }
    ~TimedLaunch() noexcept(false) { t.end(on, s); }
};

inline void check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("launch of %s failed: %s", what, hipGetErrorString(e));
        throw Error{DI_EHIP};
    }
}

// A kernel that takes more than 64 KiB of dynamic LDS must opt in
// (hipFuncAttributeMaxDynamicSharedMemorySize): once per kernel and device, not per launch.
// `set_on` is the call site's static for `kernels`, one bit per device (a device past 63
// sets the limit at every call).
struct DynLds {
    const void *kern;
    int bytes;
};
inline void dynamic_lds_once(std::atomic<uint64_t> &set_on, std::initializer_list<DynLds> kernels) {
    int dev = 0;
    DI_HIP(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? 1ull << dev : 0;
    if (set_on.load(std::memory_order_acquire) & bit) return;
    int lds_max = 0;
    DI_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    for (const DynLds &k : kernels) {
        DI_REQUIRE(k.bytes <= lds_max, DI_ERANGE,
                   "a kernel needs %d bytes of LDS per workgroup, device %d has %d", k.bytes, dev,
                   lds_max);
        DI_HIP(hipFuncSetAttribute(k.kern, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
    }
    set_on.fetch_or(bit, std::memory_order_release);
}

// The current device set to `dev` for a scope, and put back after it.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        DI_HIP(hipGetDevice(&prev));
        if (prev != dev) DI_HIP(hipSetDevice(dev));
    }
    DeviceScope(const DeviceScope &) = delete;
    ~DeviceScope() {
        int cur;
        if (hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

inline void check_device(int device) {
    int ndev = 0;
    DI_REQUIRE(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, DI_ENODEV, "no HIP device");
    DI_REQUIRE(device >= 0 && device < ndev, DI_EINVAL, "bad device %d", device);
}

// The `n` elements at a host or device pointer, as a device array: a device pointer (or
// nothing) as it is, a host array copied into `buf` on stream s.
template <class T>
const T *stage_in(const T *src, size_t n, bool device_ptrs, DevBuf &buf, hipStream_t s) {
    if (device_ptrs || n == 0) return src;
    buf.reserve(n * sizeof(T));
    DI_HIP(hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
    return buf.as<T>();
}

// An output array of the caller's.  d is where kernels write it: the caller's own pointer
// when that is a device one, else `buf`, which copy_back() copies to the caller's host
// array.  The element count may come later than the constructor, through size().
template <class T>
struct StagedOut {
    T *out, *d = nullptr;
    size_t n = 0;
    bool dev;
    DevBuf &buf;
    StagedOut(T *out_, bool dev_, DevBuf &buf_) : out(out_), dev(dev_), buf(buf_) {}
    StagedOut(T *out_, size_t n_, bool dev_, DevBuf &buf_) : StagedOut(out_, dev_, buf_) {
        size(n_);
    }
    T *size(size_t n_) {
        n = n_;
        if (dev || !out) return d = out;  // (an optional output left out stays null)
        buf.reserve(n * sizeof(T));
        return d = buf.as<T>();
    }
    void copy_back(hipStream_t s) const {  // (enqueued: the caller waits for s)
        if (!dev && out && n) DI_HIP(hipMemcpyAsync(out, d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    }
};

// One value or one small fixed array read from the device on stream s: waits for s, and
// resolves `timer` after the wait when one is given.
template <class T>
void read_back(T &host, const void *d_src, hipStream_t s, Timer *timer = nullptr) {
    static_assert(std::is_trivially_copyable<T>::value, "read_back copies bytes");
    DI_HIP(hipMemcpyAsync(&host, d_src, sizeof(T), hipMemcpyDeviceToHost, s));
    DI_HIP(hipStreamSynchronize(s));
    if (timer) timer->resolve();
}

// The n + 1 offsets `cu` of n segments, checked on the host: cu[0] == 0, none decreases,
// and no segment is longer than `cap` (when cap >= 0).  -> cu[n], the total.
template <class I>
int64_t check_cu(const I *cu, int64_t n, const char *name, int64_t cap = -1) {
    DI_REQUIRE(cu[0] == 0, DI_EINVAL, "%s[0] must be 0", name);
    for (int64_t i = 0; i < n; ++i) {
        DI_REQUIRE(cu[i + 1] >= cu[i], DI_EINVAL, "%s not monotone at %lld", name, (long long)i);
        const int64_t len = (int64_t)cu[i + 1] - (int64_t)cu[i];  // (both >= 0 here)
        DI_REQUIRE(cap < 0 || len <= cap, DI_ERANGE, "%s: segment %lld has %lld entries > %lld",
                   name, (long long)i, (long long)len, (long long)cap);
    }
    return (int64_t)cu[n];
}

// The n + 1 offsets `cu` where the host can read them: a host array as it is, a device
// array copied into `h` on stream s (waits for s).
template <class I>
const I *host_cu(const I *cu, int64_t n, bool device_ptrs, std::vector<I> &h, hipStream_t s) {
    if (!device_ptrs) return cu;
    h.resize((size_t)n + 1);
    DI_HIP(hipMemcpyAsync(h.data(), cu, h.size() * sizeof(I), hipMemcpyDeviceToHost, s));
    DI_HIP(hipStreamSynchronize(s));
    return h.data();
}

// `buf` with room for `need` bytes, its first `used` bytes kept.  Waits for s.
inline void grow_keep(DevBuf &buf, size_t need, size_t used, hipStream_t s) {
    if (need <= buf.bytes && buf.p) return;
    const size_t bytes = std::max(need, 2 * buf.bytes);
    void *p = nullptr;
    DI_HIP(hipMalloc(&p, bytes));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(p, buf.p, used, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(p);
        DI_HIP(e);
    }
    if (buf.p) (void)hipFree(buf.p);
    buf.p = p;
    buf.bytes = bytes;
}

}  // namespace di
