// octpt_stage.h -- host staging of an entry's buffers: the host-pointer form of an entry names its buffers here and
// calls its device form on the context's stream.  Host code only (no .hip file includes it).
//
//   HostStage hs(ctx->stream);
//   const float *d_in = hs.in(in, n);        // uploads first ...
//   float *d_out = hs.out(out, n);           // ... then the outputs
//   if (hs.ok() && (st = entry_device(ctx, ..., d_in, d_out, ctx->stream)) != OCTPT_OK) return st;
//   if (hs.finish() != hipSuccess) return hip_fail(ctx, hs.error(), "entry");
//
// Copies are blocking hipMemcpy.  The first HIP error is latched and every later step is a no-op, so nothing is
// downloaded after a failure; an entry that returns early (its device form's status) downloads nothing either.  The
// destructor frees every device buffer on every path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace octpt {

class HostStage {
public:
    explicit HostStage(hipStream_t stream) : stream_(stream) {}
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage() {
        for (void *p : allocs_) (void)hipFree(p);
    }

    // `count` elements of the caller's, uploaded; a NULL host pointer gives a NULL device pointer and no allocation
    template <class T>
    T *in(const T *host, size_t count) {
        return static_cast<T *>(host ? stage(host, nullptr, count * sizeof(T)) : nullptr);
    }
    // an output of `count` elements, downloaded by finish(); NULL as in()
    template <class T>
    T *out(T *host, size_t count) {
        return static_cast<T *>(host ? stage(nullptr, host, count * sizeof(T)) : nullptr);
    }
    // an output the device form always needs; downloaded only when the caller takes it (host not NULL)
    template <class T>
    T *scratch_out(T *host, size_t count) {
        return static_cast<T *>(stage(nullptr, host, count * sizeof(T)));
    }
    // src uploaded, the device form works in place, the result downloaded to dst (which may be src, or NULL: no
    // download); a NULL src as in()
    template <class T>
    T *inout(const T *src, T *dst, size_t count) {
        return static_cast<T *>(src ? stage(src, dst, count * sizeof(T)) : nullptr);
    }

    bool ok() const { return e_ == hipSuccess; }
    hipError_t error() const { return e_; }
    // a HIP call of the entry's own between its device form and finish() (a launch on the stream)
    void note(hipError_t e) {
        if (ok()) e_ = e;
    }
    // the stream drained, then the downloads in registration order
    hipError_t finish() {
        if (ok()) e_ = hipStreamSynchronize(stream_);
        for (const Download &d : downloads_)
            if (ok()) e_ = hipMemcpy(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost);
        downloads_.clear();
        return e_;
    }

private:
    struct Download {
        void *host, *dev;
        size_t bytes;
    };
    void *stage(const void *src, void *dst, size_t bytes) {
        if (!ok()) return nullptr;
        allocs_.push_back(nullptr);  // (first: a failed push_back leaks nothing)
        void *&d = allocs_.back();
        if ((e_ = hipMalloc(&d, bytes)) != hipSuccess) return d = nullptr;
        if (src) e_ = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        if (dst) downloads_.push_back({dst, d, bytes});
        return d;
    }

    hipStream_t stream_;
    hipError_t e_ = hipSuccess;
    std::vector<void *> allocs_;
    std::vector<Download> downloads_;
};

}  // namespace octpt
