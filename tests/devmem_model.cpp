// devmem_model.cpp -- the owner of device memory and the pack of csrc/lbm_devmem.hpp, and the two table sets that go through the pack
// (body_parts of csrc/lbm_bodies.hpp, motion_parts of csrc/lbm_wall_motion.hpp), driven without a device for tests/test_devmem_cpu.py.
// The device is host memory that counts its live allocations and fails on demand: the n-th alloc or the n-th copy from now on.
//   devmem_model owner            the cases of the owner and of the pack; prints "ok <case>" per case, "live <n>" at the end
//   devmem_model tables <file>    the parts of both table sets for the case in <file> (the format of wall_motion_model.cpp: nx ny
//                                 nbodies, mask, labels, then x0 y0 Ux Uy Om per body), as a batch of two equal lattices, read back
//                                 from the "device" after upload(); prints, doubles as hexadecimal floating-point numbers,
//       link x y k / chunk begin n body / maxchunks m / first f.. / centre x0 y0 / reserved partial_bytes rec_bytes / offsets o..
//       refusal r lattice S A links / cell i row / delta32 i d_1 .. d_8 / delta64 i d_1 .. d_8 / link_delta d / motion_offsets o..
//       setter <what> ...         a setter-shaped sequence: the next tables are built aside, the upload fails, the previous stay
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lbm_wall_motion.hpp"

using namespace lbmhost;

struct TestMem {
    static constexpr const char *ALLOC = "hipMalloc", *COPY = "hipMemcpy";
    static int live, frees, fail_alloc, fail_copy;   // fail_*: 1 = the next one fails, 0 = none
    static const char* alloc(void** p, size_t bytes) {
        if (fail_alloc > 0 && --fail_alloc == 0) return "out of memory";
        *p = std::malloc(bytes ? bytes : 1);
        ++live;
        return nullptr;
    }
    static void free(void* p) {
        std::free(p);
        --live;
        ++frees;
    }
    static const char* copy(void* dst, const void* src, size_t bytes) {
        if (fail_copy > 0 && --fail_copy == 0) return "invalid argument";
        std::memcpy(dst, src, bytes);
        return nullptr;
    }
};
int TestMem::live = 0, TestMem::frees = 0, TestMem::fail_alloc = 0, TestMem::fail_copy = 0;
using Buf = DevMem<TestMem>;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void owner_cases() {
    {   // alloc: success, then a failure that leaves the owner empty and names the buffer
        Buf b;
        CHECK(!b && b.get() == nullptr && b.bytes() == 0);
        CHECK(b.alloc(64, "staging").empty() && b && b.bytes() == 64 && TestMem::live == 1);
        std::memset(b.get(), 0x5a, 64);   // (the sanitizer checks the size)
        CHECK(b.as<char>() == b.get());
        TestMem::fail_alloc = 1;
        const std::string e = b.alloc(128, "staging");
        CHECK(e == "hipMalloc(staging): out of memory");
        CHECK(!b && b.bytes() == 0 && TestMem::live == 0);
        Buf never;
        TestMem::fail_alloc = 1;
        CHECK(never.alloc(8, "lattice") == "hipMalloc(lattice): out of memory" && !never && TestMem::live == 0);
    }
    CHECK(TestMem::live == 0);
    std::printf("ok alloc\n");
    {   // ensure: keeps what is large enough, replaces what is not
        Buf b;
        CHECK(b.ensure(100, "x").empty());
        void* first = b.get();
        const int frees = TestMem::frees;
        CHECK(b.ensure(100, "x").empty() && b.ensure(40, "x").empty() && b.get() == first && b.bytes() == 100 && TestMem::frees == frees);
        CHECK(b.ensure(101, "x").empty() && b.bytes() == 101 && TestMem::frees == frees + 1 && TestMem::live == 1);
        std::memset(b.get(), 1, 101);
        TestMem::fail_alloc = 1;
        CHECK(b.ensure(500, "x") == "hipMalloc(x): out of memory" && !b && TestMem::live == 0);
        CHECK(b.ensure(0, "x").empty() && b.ensure(0, "x").empty() && TestMem::live == 1);   // (no bytes: allocated once, kept)
    }
    CHECK(TestMem::live == 0);
    std::printf("ok ensure\n");
    {   // release, twice
        Buf b;
        CHECK(b.alloc(16, "x").empty());
        const int frees = TestMem::frees;
        b.release();
        b.release();
        CHECK(!b && TestMem::frees == frees + 1 && TestMem::live == 0);
        Buf empty;
        empty.release();
        CHECK(TestMem::frees == frees + 1);
    }
    std::printf("ok release\n");
    {   // moves: the source is empty afterwards, the overwritten buffer is freed once
        Buf a, b;
        CHECK(a.alloc(16, "a").empty() && b.alloc(32, "b").empty() && TestMem::live == 2);
        void* pb = b.get();
        const int frees = TestMem::frees;
        a = std::move(b);
        CHECK(a.get() == pb && a.bytes() == 32 && !b && b.bytes() == 0 && TestMem::frees == frees + 1 && TestMem::live == 1);
        Buf c(std::move(a));
        CHECK(c.get() == pb && c.bytes() == 32 && !a && TestMem::frees == frees + 1 && TestMem::live == 1);
        Buf& self = c;
        c = std::move(self);
        CHECK(c.get() == pb && TestMem::live == 1);
        c = Buf{};
        CHECK(!c && TestMem::frees == frees + 2 && TestMem::live == 0);
    }
    std::printf("ok move\n");
    {   // destruction frees
        const int frees = TestMem::frees;
        {
            Buf b;
            CHECK(b.alloc(8, "x").empty() && TestMem::live == 1);
        }
        CHECK(TestMem::frees == frees + 1 && TestMem::live == 0);
    }
    std::printf("ok destroy\n");
    {   // the pack: an empty first part, an empty part in the middle, a part that is only reserved
        const char a[5] = {1, 2, 3, 4, 5};
        std::vector<double> d(7, 0.25);
        const char z[33] = "abcdefghijklmnopqrstuvwxyz012345";
        const std::vector<Part> parts = {{nullptr, 0}, {a, sizeof a}, {a, 0}, {d.data(), d.size() * sizeof(double)}, {nullptr, 40}, {z, sizeof z}};
        Pack<TestMem> p = upload<TestMem>(parts, "tables");
        CHECK(p.err.empty() && !p.no_memory && p.buf && TestMem::live == 1);
        size_t end = 0;
        for (size_t i = 0; i < parts.size(); ++i) {
            CHECK(p.off[i] % 16 == 0 && p.off[i] >= end);
            end = p.off[i] + parts[i].bytes;
        }
        CHECK(end <= p.buf.bytes());
        CHECK(std::memcmp(p.at<char>(1), a, sizeof a) == 0 && std::memcmp(p.at<double>(3), d.data(), d.size() * sizeof(double)) == 0 &&
              std::memcmp(p.at<char>(5), z, sizeof z) == 0);
        std::memset(p.at<char>(4), 0x33, 40);   // the reserved part is the caller's to write
        CHECK(std::memcmp(p.at<char>(5), z, sizeof z) == 0 && std::memcmp(p.at<double>(3), d.data(), d.size() * sizeof(double)) == 0);
        Pack<TestMem> none = upload<TestMem>({{nullptr, 0}, {a, 0}}, "nothing");   // nothing at all is still an allocation
        CHECK(none.err.empty() && none.buf && none.off[0] == 0 && none.off[1] == 0 && TestMem::live == 2);
        // a failing copy frees; a failing allocation says so
        for (int nth = 1; nth <= 3; ++nth) {
            TestMem::fail_copy = nth;
            Pack<TestMem> bad = upload<TestMem>(parts, "tables");
            CHECK(bad.err == "hipMemcpy(tables): invalid argument" && !bad.no_memory && !bad.buf && TestMem::live == 2);
        }
        TestMem::fail_copy = 4;   // (three copies only: none fails)
        CHECK(upload<TestMem>(parts, "tables").err.empty());
        TestMem::fail_copy = 0;
        TestMem::fail_alloc = 1;
        Pack<TestMem> nomem = upload<TestMem>(parts, "tables");
        CHECK(nomem.err == "hipMalloc(tables): out of memory" && nomem.no_memory && !nomem.buf && TestMem::live == 2);
    }
    CHECK(TestMem::live == 0);
    std::printf("ok pack\n");
}

// ---- the two table sets ----
struct Case {
    int nx = 0, ny = 0, nb = 0;
    std::vector<uint8_t> mask;      // a batch of two equal lattices
    std::vector<int32_t> label;
    std::vector<double> centre, motion;
};
static bool read_case(const char* path, Case& k) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return false;
    if (std::fscanf(f, "%d %d %d", &k.nx, &k.ny, &k.nb) != 3 || k.nx < 1 || k.ny < 1 || k.nb < 1 || k.nb > BODY_MAX) return false;
    const size_t n = (size_t)k.nx * k.ny;
    k.mask.resize(2 * n);
    k.label.resize(2 * n);
    for (size_t i = 0; i < n; ++i) {
        int v = 0;
        if (std::fscanf(f, "%d", &v) != 1) return false;
        k.mask[i] = k.mask[n + i] = (uint8_t)v;
    }
    for (size_t i = 0; i < n; ++i) {
        if (std::fscanf(f, "%d", &k.label[i]) != 1) return false;
        k.label[n + i] = k.label[i];
    }
    k.centre.resize(4 * (size_t)k.nb);
    k.motion.resize(6 * (size_t)k.nb);
    for (int b = 0; b < k.nb; ++b) {
        double* c = &k.centre[2 * b];
        double* m = &k.motion[3 * b];
        if (std::fscanf(f, "%la %la %la %la %la", c, c + 1, m, m + 1, m + 2) != 5) return false;
        for (int j = 0; j < 2; ++j) k.centre[2 * (k.nb + b) + j] = c[j];
        for (int j = 0; j < 3; ++j) k.motion[3 * (k.nb + b) + j] = m[j];
    }
    std::fclose(f);
    return true;
}

// What a setter keeps: the tables the context holds, as an owner and a view into it.
struct Held {
    Buf base;
    const char* view = nullptr;
};
// "build next, upload, commit": on a failure `held` is what it was
template <typename Parts>
static bool set_tables(Held& held, const Parts& next, const char* what, std::string& err) {
    Pack<TestMem> p = upload<TestMem>(next.parts(), what);
    if (!p.err.empty()) {
        err = p.err;
        return false;
    }
    held.view = p.template at<const char>(0);
    held.base = std::move(p.buf);
    return true;
}

static int tables(const char* path) {
    Case k;
    if (!read_case(path, k)) return 2;
    const int ACC = 4, REC = 6;
    const size_t n = (size_t)k.nx * k.ny;
    {
        const BodyParts t = body_parts(k.mask.data(), k.label.data(), k.centre.data(), 2, k.nx, k.ny, k.nb, ACC, REC);
        Pack<TestMem> p = upload<TestMem>(t.parts(), "body tables");
        if (!p.err.empty()) return 3;
        const BodyLink* links = p.at<const BodyLink>(BodyParts::LINKS);
        for (size_t i = 0; i < t.links.size(); ++i) std::printf("link %d %d %d\n", links[i].x, links[i].yk >> 4, links[i].yk & 15);
        const BodyChunk* chunks = p.at<const BodyChunk>(BodyParts::CHUNKS);
        for (size_t i = 0; i < t.chunks.size(); ++i) std::printf("chunk %lld %d %d\n", chunks[i].begin, chunks[i].n, chunks[i].body);
        std::printf("maxchunks %zu\nfirst", t.maxchunks);
        const int32_t* first = p.at<const int32_t>(BodyParts::FIRST);
        for (size_t i = 0; i < t.first.size(); ++i) std::printf(" %d", first[i]);
        std::printf("\n");
        const double* centre = p.at<const double>(BodyParts::CENTRE);
        for (int i = 0; i < 2 * k.nb; ++i) std::printf("centre %a %a\n", centre[2 * i], centre[2 * i + 1]);
        std::printf("reserved %zu %zu\noffsets", t.partial_bytes, t.rec_bytes);
        for (size_t o : p.off) std::printf(" %zu", o);
        std::printf("\n");
        std::memset(p.at<char>(BodyParts::PARTIAL), 0, t.partial_bytes);   // (inside the allocation: the sanitizer checks)
        std::memset(p.at<char>(BodyParts::REC), 0, t.rec_bytes);
    }
    for (int f32 = 1; f32 >= 0; --f32) {
        const MotionParts t = motion_parts(k.mask.data(), k.label.data(), k.centre.data(), k.motion.data(), 2, k.nx, k.ny, k.nb, f32 != 0);
        if (f32) std::printf("refusal %d %d %a %a %zu\n", (int)t.refusal, t.lattice, t.S, t.A, t.links);
        if (t.refusal != MotionParts::NONE) break;
        Pack<TestMem> p = upload<TestMem>(t.parts(), "body motion tables");
        if (!p.err.empty()) return 3;
        const size_t rows = t.delta.size() / 8 / (f32 ? 4 : 8);
        if (f32) {
            const int32_t* cell_row = p.at<const int32_t>(MotionParts::CELL_ROW);
            for (size_t i = 0; i < 2 * n; ++i)
                if (cell_row[i] >= 0) std::printf("cell %zu %d\n", i, cell_row[i]);
            const double* ld = p.at<const double>(MotionParts::LINK_DELTA);
            for (size_t i = 0; i < t.link_delta.size(); ++i) std::printf("link_delta %a\n", ld[i]);
            std::printf("motion_offsets");
            for (size_t o : p.off) std::printf(" %zu", o);
            std::printf("\n");
        }
        for (size_t r = 0; r < rows; ++r) {
            std::printf(f32 ? "delta32 %zu" : "delta64 %zu", r);
            for (int j = 0; j < 8; ++j) std::printf(" %a", f32 ? (double)p.at<const float>(MotionParts::DELTA)[8 * r + j] : p.at<const double>(MotionParts::DELTA)[8 * r + j]);
            std::printf("\n");
        }
    }
    // The setter-shaped sequences: tables are held; the next ones are built aside and their upload fails (the allocation, then each
    // copy); what is held is still the first tables, byte for byte, and nothing else is live.
    {
        const BodyParts first = body_parts(k.mask.data(), k.label.data(), k.centre.data(), 2, k.nx, k.ny, k.nb, ACC, REC);
        std::vector<int32_t> relabel(k.label);
        for (int32_t& v : relabel) v = v > 0 ? 0 : v;
        const BodyParts next = body_parts(k.mask.data(), relabel.data(), k.centre.data(), 2, k.nx, k.ny, k.nb, ACC, REC);
        Held held;
        std::string err;
        bool kept = set_tables(held, first, "body tables", err);
        auto still_first = [&] {
            return TestMem::live == 1 && held.view == held.base.as<const char>() &&
                   std::memcmp(held.view, first.links.data(), first.links.size() * sizeof(BodyLink)) == 0;
        };
        int copies = 0, refused = 0;
        for (const Part& q : next.parts()) copies += q.src && q.bytes ? 1 : 0;
        TestMem::fail_alloc = 1;
        refused += !set_tables(held, next, "body tables", err) && err == "hipMalloc(body tables): out of memory" ? 1 : 0;
        kept = kept && still_first();
        for (int nth = 1; nth <= copies; ++nth) {
            TestMem::fail_copy = nth;
            refused += !set_tables(held, next, "body tables", err) && err == "hipMemcpy(body tables): invalid argument" ? 1 : 0;
            kept = kept && still_first();
        }
        TestMem::fail_copy = 0;
        std::printf("setter bodies failures %d refused %d kept %d live %d\n", copies + 1, refused, kept ? 1 : 0, TestMem::live);
        const bool committed = set_tables(held, next, "body tables", err) && TestMem::live == 1 &&
                               std::memcmp(held.view, next.links.data(), next.links.size() * sizeof(BodyLink)) == 0;
        std::printf("setter bodies committed %d live %d\n", committed ? 1 : 0, TestMem::live);
    }
    std::printf("setter bodies end live %d\n", TestMem::live);
    {
        const MotionParts first = motion_parts(k.mask.data(), k.label.data(), k.centre.data(), k.motion.data(), 2, k.nx, k.ny, k.nb, true);
        if (first.refusal == MotionParts::NONE) {
            std::vector<double> faster(k.motion);
            for (double& v : faster) v *= 2.0;
            const MotionParts next = motion_parts(k.mask.data(), k.label.data(), k.centre.data(), faster.data(), 2, k.nx, k.ny, k.nb, true);
            Held held;
            std::string err;
            bool same = set_tables(held, first, "body motion tables", err);
            TestMem::fail_copy = 1;
            const bool refused = !set_tables(held, next, "body motion tables", err) && err == "hipMemcpy(body motion tables): invalid argument";
            TestMem::fail_copy = 0;
            same = same && TestMem::live == 1 && std::memcmp(held.view, first.cell_row.data(), first.cell_row.size() * sizeof(int32_t)) == 0;
            std::printf("setter motion refused %d kept %d live %d\n", refused ? 1 : 0, same ? 1 : 0, TestMem::live);
        }
    }
    std::printf("setter motion end live %d\n", TestMem::live);
    return 0;
}

int main(int argc, char** argv) {
    int rc = 2;
    if (argc == 2 && std::strcmp(argv[1], "owner") == 0) {
        owner_cases();
        rc = failures ? 1 : 0;
    } else if (argc == 3 && std::strcmp(argv[1], "tables") == 0) {
        rc = tables(argv[2]);
    }
    std::printf("live %d\n", TestMem::live);
    return rc;
}
