// Host-only check of the runtime's shared point-to-point argument helpers (check_pe, peer_range,
// peer_address, check_sig_op, sync_word_error, rma_args): the boundary cases, against the literal
// messages the entry points reported before the helpers existed.  The helpers are internal to
// runtime.cpp, so this program compiles that file into itself and fills a State by hand: a fake
// 4 KiB "heap" (the helpers only do pointer arithmetic on it) of a 2-PE job.  No HIP call is made,
// so it runs without a GPU.  Prints "p2p_checks OK" and exits 0, or lists what differed.
#include "../../ishmem_amd/csrc/runtime.cpp"

namespace {

int g_bad = 0;

void expect_msg(const char *label, bool failed, const char *want)
{
    const std::string got = failed ? ishmemi_c_last_error() : "(accepted)";
    if (got != want) {
        printf("MISMATCH %s\n  got : %s\n  want: %s\n", label, got.c_str(), want);
        ++g_bad;
    }
}

void expect_true(const char *label, bool ok)
{
    if (!ok) {
        printf("MISMATCH %s\n", label);
        ++g_bad;
    }
}

}  // namespace

int main()
{
    State &s = S();
    alignas(256) static char heap[4096], peer[4096];
    s.heap = heap;
    s.heap_size = sizeof(heap);
    s.pe = 0;
    s.npes = 2;
    s.peer_heap[1] = peer;

    // PE range: -1 and npes are refused, 0 and npes - 1 accepted.
    expect_msg("pe -1", check_pe(s, "put", -1), "put: pe -1 outside [0, 2)");
    expect_msg("pe npes", check_pe(s, "get_nbi", 2), "get_nbi: pe 2 outside [0, 2)");
    expect_msg("pe 0", check_pe(s, "put", 0), "(accepted)");
    expect_msg("pe npes - 1", check_pe(s, "put", 1), "(accepted)");

    // A range ending exactly at the heap's end is inside, one byte more is not; so is a start outside.
    expect_true("range to the end, own PE", peer_range(s, "put", "dest", "length", heap + 96, 4000, 0) == heap + 96);
    expect_true("range to the end, peer", peer_range(s, "put", "dest", "length", heap + 96, 4000, 1) == peer + 96);
    expect_msg("one byte past the end", !peer_range(s, "put", "dest", "length", heap + 96, 4001, 1),
               "put: dest is not inside the symmetric heap for its whole length");
    expect_msg("extent past the end", !peer_range(s, "ibget_on_stream", "source", "extent", heap, 4097, 1),
               "ibget_on_stream: source is not inside the symmetric heap for its whole extent");
    expect_msg("start at the end", !peer_range(s, "get", "source", "length", heap + 4096, 1, 1),
               "get: source is not inside the symmetric heap for its whole length");
    expect_msg("start outside the heap", !peer_range(s, "get", "source", "length", &g_bad, 1, 1),
               "get: source is not inside the symmetric heap for its whole length");
    expect_msg("huge length", !peer_range(s, "put", "dest", "length", heap, ~0ull, 1),
               "put: dest is not inside the symmetric heap for its whole length");

    // A peer whose heap is not mapped here.
    s.peer_heap[1] = nullptr;
    expect_msg("peer not mapped (range)", !peer_range(s, "put", "dest", "length", heap, 8, 1), "put: heap of PE 1 not mapped");
    expect_msg("peer not mapped (word)", !peer_address(s, "atomic_fetch_add", heap, 1), "atomic_fetch_add: heap of PE 1 not mapped");
    s.peer_heap[1] = peer;

    // Signal words: null, misaligned, outside, the last word of the heap.
    auto sig = [&](const void *p, size_t w) {
        const char *e = sync_word_error(s, p, w);
        return std::string("put_signal: sig_addr") + (e ? e : " ok");
    };
    expect_true("null signal word", sig(nullptr, 8) == "put_signal: sig_addr is null");
    expect_true("misaligned signal word", sig(heap + 4, 8) == "put_signal: sig_addr is not 8-byte aligned");
    expect_true("misaligned 4-byte word", sig(heap + 2, 4) == "put_signal: sig_addr is not 4-byte aligned");
    expect_true("signal word past the end", sig(heap + 4096, 8) == "put_signal: sig_addr is not inside the symmetric heap");
    expect_true("last signal word", sig(heap + 4088, 8) == "put_signal: sig_addr ok");
    expect_true("4-byte word at 4092", sig(heap + 4092, 4) == "put_signal: sig_addr ok");

    expect_msg("sig_op set", check_sig_op("signal_op", kSignalSet), "(accepted)");
    expect_msg("sig_op add", check_sig_op("signal_op", kSignalAdd), "(accepted)");
    expect_msg("sig_op 7", check_sig_op("put_signal_nbi", 7),
               "put_signal_nbi: sig_op 7 is neither ISHMEM_SIGNAL_SET nor ISHMEM_SIGNAL_ADD");

    // The 16-byte split: head bytes up to dest's next boundary, whole items, the rest.
    for (size_t off = 0; off < 32; ++off)
        for (size_t n : {(size_t) 0, (size_t) 1, (size_t) 15, (size_t) 16, (size_t) 17, (size_t) 100}) {
            const RmaArgs a = rma_args(heap + off, peer, n);
            size_t head = 0;
            while (head < n && ((uintptr_t) (heap + off + head) & 15)) ++head;
            expect_true("rma_args", a.dst == heap + off && a.src == peer && a.head == head && a.nitems == (n - head) / 16 &&
                                        a.head + a.nitems * 16 + a.tail == n && a.tail < 16);
        }

    if (g_bad) return 1;
    printf("p2p_checks OK\n");
    return 0;
}
