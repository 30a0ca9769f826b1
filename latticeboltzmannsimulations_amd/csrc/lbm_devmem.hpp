// lbm_devmem.hpp -- who owns device memory: DevMem, one allocation that frees itself, and upload(), several host tables in one
// allocation.  The device is the parameter Mem (lbm_host.hpp: HipMem), which provides
//     static const char* alloc(void** p, size_t bytes), copy(void* dst, const void* src, size_t bytes)   null, or the error's text
//     static void free(void* p)
//     static constexpr const char *ALLOC, *COPY                                                          the calls' names, for the messages
// Plain C++, nothing from HIP: tests/test_devmem_cpu.py drives it from a program of its own, with a Mem that counts and fails on demand.
#pragma once
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

namespace lbmhost {

// One allocation, or none.  Move-only; what it holds is freed when it is overwritten, released or destroyed.
template <typename Mem>
class DevMem {
    void* p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) {
            release();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~DevMem() { release(); }

    // A fresh allocation in place of what was held: "" or, the owner empty, "<ALLOC>(<what>): <the error's text>".
    std::string alloc(size_t bytes, const char* what) {
        release();
        if (const char* e = Mem::alloc(&p_, bytes)) {
            p_ = nullptr;
            return std::string(Mem::ALLOC) + "(" + what + "): " + e;
        }
        bytes_ = bytes;
        return "";
    }
    // Allocated on first use, kept: what is held stays when it is large enough and is replaced (not copied) when it is not.
    std::string ensure(size_t bytes, const char* what) { return p_ && bytes_ >= bytes ? "" : alloc(bytes, what); }
    void release() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }

    void* get() const { return p_; }
    template <typename T>
    T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }
    size_t bytes() const { return bytes_; }
};

// One table of a pack: `bytes` bytes copied from src, or only reserved (src null).  No bytes at all is legal.
struct Part {
    const void* src;
    size_t bytes;
};
constexpr size_t PACK_ALIGN = 16;
// Where the parts lie, each at the next multiple of PACK_ALIGN; *total: the bytes of the allocation (never 0).
inline std::vector<size_t> pack_offsets(const std::vector<Part>& parts, size_t* total) {
    std::vector<size_t> off(parts.size());
    size_t at = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        off[i] = at;
        at += (parts[i].bytes + PACK_ALIGN - 1) / PACK_ALIGN * PACK_ALIGN;
    }
    *total = at ? at : PACK_ALIGN;
    return off;
}

// What upload() hands back: the allocation and the parts' offsets in it, or, buf empty, the error (no_memory: of the allocation).
template <typename Mem>
struct Pack {
    DevMem<Mem> buf;
    std::vector<size_t> off;
    std::string err;
    bool no_memory = false;
    template <typename T>
    T* at(size_t part) const { return reinterpret_cast<T*>(buf.template as<char>() + off[part]); }
};
// One allocation for all parts, those with a source copied into it.  A failed copy frees it: "<COPY>(<what>): <the error's text>".
template <typename Mem>
Pack<Mem> upload(const std::vector<Part>& parts, const char* what) {
    Pack<Mem> p;
    size_t total = 0;
    p.off = pack_offsets(parts, &total);
    p.err = p.buf.alloc(total, what);
    p.no_memory = !p.err.empty();
    for (size_t i = 0; i < parts.size() && p.err.empty(); ++i) {
        if (!parts[i].src || !parts[i].bytes) continue;
        if (const char* e = Mem::copy(p.template at<char>(i), parts[i].src, parts[i].bytes)) p.err = std::string(Mem::COPY) + "(" + what + "): " + e;
    }
    if (!p.err.empty()) p.buf.release();
    return p;
}
}  // namespace lbmhost
