// diasss_amd/host/ctx_buffers_check.cpp -- the failure path of the context's buffer ownership (csrc/dsss_internal.h: dsss_buf,
// dsss_family_alloc, dsss_ensure_store), exercised WITHOUT a device: there every hipMalloc / hipHostMalloc fails, which makes the
// path no GPU test may provoke free and deterministic.  Built with the host sanitizers (Makefile: ctx_buffers_check), linked against
// libdsss.so for dsss_ensure_store.  Exit status: 0 all checks hold, 1 one does not, 77 a device is present (nothing was checked).
#include "../csrc/dsss_internal.h"

static int g_fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); ++g_fails; } } while (0)

static char g_dummy[64];      // stands for a block the buffer held before: never dereferenced, and no runtime without a device frees anything

static void check_reserve(bool pinned)
{
    dsss_ctx c;
    dsss_buf b("b", pinned);
    CHECK(b.reserve(&c, 0) == DSSS_OK && !b && b.cap == 0 && c.err.empty());      // nothing needed: no call into the runtime
    CHECK(b.reserve(&c, 256, 512) == DSSS_E_HIP);
    CHECK(b.p == nullptr && b.cap == 0 && c.err.find("b: ") == 0);                 // dsss_last_error names the buffer
    // ... and when it held a block before
    dsss_buf held("held", pinned); held.p = g_dummy; held.cap = 16;
    dsss_buf m(std::move(held));
    CHECK(held.p == nullptr && held.cap == 0 && m.p == g_dummy && m.cap == 16 && m.pinned == pinned);
    CHECK(m.reserve(&c, 16) == DSSS_OK && m.p == g_dummy);                          // below capacity: untouched
    c.err.clear();
    CHECK(m.reserve(&c, 64) == DSSS_E_HIP);
    CHECK(m.p == nullptr && m.cap == 0 && !c.err.empty());
    CHECK(m.as<double>() == nullptr);
    // reserve_keep: a failure leaves the buffer as it was
    dsss_buf k("k", pinned); k.p = g_dummy; k.cap = 16; c.err.clear();
    CHECK(k.reserve_keep(&c, 64, 96, 16) == DSSS_E_HIP);
    CHECK(k.p == g_dummy && k.cap == 16 && !c.err.empty());
    k.p = nullptr; k.cap = 0;
}

static void check_moves()
{
    dsss_buf a("a", DSSS_PINNED); a.release(); a.release(); // idempotent
    dsss_buf b("b", DSSS_PINNED); b.p = g_dummy; b.cap = 8;
    dsss_buf c2(std::move(b));                              // move-construct
    CHECK(!b && c2.p == g_dummy && c2.pinned);
    a = std::move(c2);                                      // move-assign between buffers of one kind: the block moves, name and kind stay
    CHECK(!c2 && c2.cap == 0 && a.p == g_dummy && a.cap == 8 && a.pinned && a.name[0] == 'a');
    a = std::move(a);                                       // self-assignment keeps the block
    CHECK(a.p == g_dummy);
    a.release(); a.release();
    CHECK(!a && a.cap == 0);
    dsss_frame f; f.raw_owned.p = g_dummy; f.raw_owned.cap = 8;
    std::vector<dsss_frame> v(2);
    v[1] = std::move(f);                                    // a frame stays movable (dsss_ctx::frames, free_frame)
    CHECK(!f.raw_owned && v[1].raw_owned.p == g_dummy);
    v.resize(64);                                           // reallocation moves
    CHECK(v[1].raw_owned.p == g_dummy);
    v[1] = dsss_frame();
    CHECK(!v[1].raw_owned);
}                                                           // moved-from objects are destroyed here

static void check_family()
{
    dsss_ctx c;
    int* a = reinterpret_cast<int*>(g_dummy); double* b = nullptr; double* h = nullptr; size_t cap = 7;      // first member pre-set
    const std::array<dsss_fam_slot, 3> fam = {{ dsss_slot(a, 64), dsss_slot(b, 128), dsss_slot(h, 128, DSSS_PINNED) }};
    CHECK(dsss_family_alloc(&c, "fam", cap, 9, fam) == DSSS_E_HIP);
    CHECK(a == nullptr && b == nullptr && h == nullptr && cap == 0 && c.err.find("fam: ") == 0);
    dsss_family_release(cap, fam); dsss_family_release(cap, fam);
    CHECK(a == nullptr && cap == 0);
}

static void check_store()
{
    dsss_ctx c; c.max_frames = 4; c.kcap = 128;
    // (without a device the FIRST of the seven allocations fails, so this holds the return codes and the empty store; the state the old
    // code tripped over -- a family with its first member set and the rest null -- is what check_family starts from)
    for (int call = 0; call < 2; ++call) {
        c.err.clear();
        CHECK(dsss_ensure_store(&c) == DSSS_E_HIP);
        CHECK(!c.err.empty() && c.store_cap == 0);
        CHECK(!c.kps && !c.desc && !c.geo && !c.nkp_dev && !c.rows_dev && !c.cols_dev && !c.bbox_dev);
    }
    CHECK(dsss_ensure_sift_store(&c) == DSSS_E_HIP && !c.desc128 && !c.sift_w);
}

int main()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) { printf("SKIP: %d device(s) present, allocations would succeed\n", ndev); return 77; }
    (void)hipGetLastError();
    check_reserve(false); check_reserve(DSSS_PINNED);
    check_moves(); check_family(); check_store();
    printf(g_fails ? "ctx_buffers_check: %d check(s) failed\n" : "ctx_buffers_check: ok\n", g_fails);
    return g_fails ? 1 : 0;
}
