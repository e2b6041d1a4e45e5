/*
 * hq_devmem.h -- device memory of the solver library in one place: the error helpers every allocation reports through
 * (g_err, the storage behind hq_last_error(), lives here with hq_fail / HQ_HIP / HQ_TRY: hq_patch.h and hq_brick.h need them
 * ahead of the engine), the copy that is waited for on a stream of the context, and hq_dbuf<T>, the move-only owner of one
 * device array.  Included once by hq_engine.hip, ahead of hq_patch.h / hq_brick.h.
 * The rule it keeps: nothing the steps read goes through the null stream.  The context's streams are non-blocking, so a
 * null-stream copy or memset is not ordered with them; every upload and fill here is enqueued on the stream it is given
 * (the context's compute stream) and waited for there, so the data is in place when the call returns and the host
 * buffer may go out of scope.  A consequence for an entry point that uploads while steps are still enqueued
 * (hq_snapshot_add's map; the others -- hq_record_fetch, hq_sync, hq_set_source -- quiesce the context first, as they
 * did): the host blocks until the compute stream has drained up to the copy, where a null-stream copy slipped past the steps.
 */
#ifndef HQ_DEVMEM_H
#define HQ_DEVMEM_H

static thread_local char g_err[512] = "";

static int hq_fail(int code, const char* fmt, const char* a = "", const char* b = "")
{
    snprintf(g_err, sizeof g_err, fmt, a, b);
    return code;
}

#define HQ_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess)                                                         \
            return hq_fail(HQ_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_));    \
    } while (0)

#define HQ_TRY(x) do { int r_ = (x); if (r_ != HQ_OK) return r_; } while (0)

/* `bytes` in either direction on `st`, and they have arrived when this returns */
static int hq_copy_wait(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    if (!bytes) return HQ_OK;
    HQ_HIP(hipMemcpyAsync(dst, src, bytes, kind, st));
    HQ_HIP(hipStreamSynchronize(st));
    return HQ_OK;
}

/* one device array and the ledger (hq_ctx.bytes, or none) its bytes are counted in: they go back when the array goes */
template <typename T>
class hq_dbuf {
    T* p_ = nullptr;
    int64_t* ledger_ = nullptr;
    size_t bytes_ = 0;
public:
    hq_dbuf() = default;
    hq_dbuf(const hq_dbuf&) = delete;
    hq_dbuf& operator=(const hq_dbuf&) = delete;
    hq_dbuf(hq_dbuf&& o) noexcept : p_(o.p_), ledger_(o.ledger_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    hq_dbuf& operator=(hq_dbuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; ledger_ = o.ledger_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~hq_dbuf() { reset(); }
    void reset()
    {
        if (p_) { hipFree(p_); if (ledger_) *ledger_ -= (int64_t)bytes_; }
        p_ = nullptr; bytes_ = 0;
    }
    /* max(count, 1) elements (a table of nothing still has an address), counted in *ledger; ledger == NULL: uncounted */
    int alloc(int64_t* ledger, size_t count)
    {
        reset();
        const size_t bytes = sizeof(T) * (count ? count : 1);
        const hipError_t e = hipMalloc((void**)&p_, bytes);
        if (e != hipSuccess) {
            p_ = nullptr;
            (void)hipGetLastError();                             /* reported here: no later call finds it */
            return hq_fail(HQ_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
        }
        ledger_ = ledger; bytes_ = bytes;
        if (ledger_) *ledger_ += (int64_t)bytes_;
        return HQ_OK;
    }
    int upload(const T* host, size_t count, hipStream_t st) { return hq_copy_wait(p_, host, sizeof(T) * count, hipMemcpyHostToDevice, st); }
    int fill(int byte, hipStream_t st)
    {
        HQ_HIP(hipMemsetAsync(p_, byte, bytes_, st));
        HQ_HIP(hipStreamSynchronize(st));
        return HQ_OK;
    }
    /* allocate and upload: count elements at host, or a vector */
    int put(int64_t* ledger, const T* host, size_t count, hipStream_t st)
    {
        HQ_TRY(alloc(ledger, count));
        return upload(host, count, st);
    }
    template <typename V>
    int put(int64_t* ledger, const V& v, hipStream_t st) { return put(ledger, v.data(), v.size(), st); }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    operator T*() const { return p_; }
};

#endif /* HQ_DEVMEM_H */
