// The order-sensitive tail of the device graph build (GraphBuilder::Impl::tail): K12 sequences, K13 link order, K14 analysis, both K15
// renumberings, K17 expand_repeats, K16 finalisation and the last read-back.  Nothing in it depends on the key width, so it is compiled
// once, beside the per-width units (graph_stages.hip), and its kernels exist once in the library.
#include "graph_impl.hpp"

namespace ac {

// renumber_unitigs (unitig_graph.rs:295-315): stable sort of `order` by (length desc, sequence asc, depth desc).
[[maybe_unused]] static bool renum_two_pass() { return knobs().renum_two_pass; }      // 1: always the two-pass renumber sort
[[maybe_unused]] static u32 renum_max_group() { return knobs().renum_max_group; }      // tests: smaller groups take the fallbacks
// deferred: do not wait for the "group too large" flag (a host round trip per renumbering) — the caller reads it with the build's last
// read-back and repeats the build with checked sorts if it was ever set (GraphBuilder::build; the flag is sticky then: never cleared here).
// sc: the sort's scratch if the caller prepared it (RadixScratch); len_bits: no unitig is 2^len_bits long or longer (the keys' leading
// field is ~length: its bits above that are ones in every key and need no pass)
[[maybe_unused]] static void renumber_sort(DBuf<u32>& order, u32 U, const u32* len, const u64* off, const u8* seq, const u32* depth, u32* flag, bool deferred = false,
                                           RadixScratch* sc = nullptr, int len_bits = 32, bool order_is_identity = false) {
    if (U <= 1) return;
    DBuf<u32> backup(deferred && !renum_two_pass() ? 0 : U);      // (the order to fall back from: only a checked sort ever does)
    if (backup.size()) copy_d2d(backup.ptr(), order.ptr(), (size_t)U * 4);
    DBuf<u64> prefix(U), key(U);
    UnitigLess less{len, off, seq, depth};
    u32 zero = 0;
    if (!renum_two_pass()) {      // one sort on (length | 16 bases), ties by the comparator
        // (one kernel where `order` is still the identity — the first renumbering: element i IS unitig i and the sequences are read front to
        // back; the second renumbering's order is by length, and a fused kernel would gather its prefixes from all over the sequences:
        // mini-E's finalize stage 4.4 -> 5.7 ms when it did, r14d)
        if (order_is_identity) launch(U, RenumKeyPassFunctor{RenumKeyFunctor{len, off, seq, prefix.ptr()}, RenumPassFunctor{order.ptr(), len, depth, prefix.ptr(), 2, key.ptr()}});
        else {
            launch(U, RenumKeyFunctor{len, off, seq, prefix.ptr()});
            launch(U, RenumPassFunctor{order.ptr(), len, depth, prefix.ptr(), 2, key.ptr()});
        }
        sort_pairs_u64_u32(key, order, U, 32 + std::min(std::max(len_bits, 1), 32), 0, 0, sc);
        launch(U, RenumTieFunctor{order.ptr(), U, len, depth, prefix.ptr(), less, flag, 0, renum_max_group()});
#ifdef AC_EMU
        if (knobs().degree_diag) {
            u64 groups = 0, members = 0, biggest = 0, cur = 1, longest = 0;
            for (u32 i = 1; i <= U; i++) {
                bool same = i < U && len[order.ptr()[i]] == len[order.ptr()[i - 1]] && (prefix.ptr()[order.ptr()[i]] >> 32) == (prefix.ptr()[order.ptr()[i - 1]] >> 32);
                if (same) cur++;
                else { if (cur > 1) { groups++; members += cur; if (cur > biggest) biggest = cur; if (len[order.ptr()[i - 1]] > longest) longest = len[order.ptr()[i - 1]]; } cur = 1; }
            }
            fprintf(stderr, "renumber diag: U %u, groups %llu, members %llu, biggest %llu, longest member %llu, flag %u\n", U, (unsigned long long)groups,
                    (unsigned long long)members, (unsigned long long)biggest, (unsigned long long)longest, *flag);
        }
#endif
        if (deferred) return;
        if (!read_scalar(flag)) return;
        copy_d2d(order.ptr(), backup.ptr(), (size_t)U * 4);      // a large group of unitigs sharing length and 16 bases: the two-pass form
        copy_h2d(flag, &zero, 4);
    }
    if (renum_two_pass()) launch(U, RenumKeyFunctor{len, off, seq, prefix.ptr()});      // (else the one-pass attempt above left the prefixes)
    for (int pass = 0; pass < 2; pass++) {
        launch(U, RenumPassFunctor{order.ptr(), len, depth, prefix.ptr(), pass, key.ptr()});
        sort_pairs_u64_u32(key, order, U, 64);
    }
    launch(U, RenumTieFunctor{order.ptr(), U, len, depth, prefix.ptr(), less, flag, 1, renum_max_group()});
    if (read_scalar(flag)) {    // a large group of long unitigs sharing length and 32-base prefix: comparator merge sort
        copy_d2d(order.ptr(), backup.ptr(), (size_t)U * 4);
        sort_keys_cmp(order, U, less);
        copy_h2d(flag, &zero, 4);
    }
}

namespace {

// Late copies (round 6): a result of the last stage is copied out behind the kernel that made it — through an event of stream 0 the side
// stream waits for (after_main), or, AC_LATE_COPIES, ISSUED BY THIS THREAD once that event has fired: it has enqueued every kernel of the
// build long before the device gets there and only waits from then on, so it can watch the events in order and hand the copy engine work
// whose inputs are ready (on some boxes a copy queue that has to wait for a kernel wakes up late: DESIGN.md §6.2, the 0.800 s builds).
struct LateCopy { void* ev; std::function<void()> issue; };
struct RemapJoin { PathRemapJob& j; ~RemapJoin() { path_remap_finish(j); } };
struct SeqJoin { SeqExpandJob& j; ~SeqJoin() { seq_expand_finish(j); } };

// One run of the tail: the state that crosses its stages, and the stages in the order run() calls them.
// Allocation order is behaviour: a DBuf is a bump-arena slice without ownership, and a stage's clears leave as ONE fused fill launch with
// its first kernel only because every buffer is allocated, cleared and every RadixScratch prepared in exactly this order.  The members
// below are therefore allocated by the stages (alloc), never where they are declared; the order of launches, read-backs and side-stream
// calls inside the stages is the build's schedule.
struct TailRun {
    GraphBuilder::Impl& m;
    FinalGraph* const out; const bool want_graph, want_paths;
    PackedText& g = *m.G;
    const u32 n_seqs = m.loc.n_seqs;
    SideStream& side = SideStream::get();
    // Destruction order is behaviour too: the members from here to rec_pos_block go in the reverse of this order, whatever ends the run.
    HostBlock number_block;      // (declared before the guard: it goes after the side stream has drained, whatever ends this scope)
    SideStream::Guard side_guard;
    PathRemapJob remap_job;
    RemapJoin remap_join{remap_job};      // (the threads are done before the guard and the table go)
    HostBlock seq_words_block; SeqExpandJob seq_job; bool seq_as_codes = false;
    std::vector<LateCopy> late;
    bool late_by_host = false;
    SeqJoin seq_join{seq_job};
    HostBlock rec_val_block, rec_pos_block;
    // path export choice
    bool host_remap = false, host_stretch = false, host_numbers = false;
    u64 n_stretch = 0, stretch_split_wave = 0;
    // cleared buffers + K12
    u64 total = 0, J = 0;
    DBuf<u8> useq, fixed_start, fixed_end, cand;
    DBuf<u32> renum_flag, cflag, pool_used;
    static const u32 SHIFT_CHECKS = 64;      // host checks of the pass loop whose "moved something" words are cleared up front (two words per check)
    DBuf<u64> shifted2, lcount, sums, n_links_dev;
    RadixScratch sort1, sort2;
    int len_bits = 32;      // no unitig is longer than the longest sequence of a text whose sequences this build knows
    // K13 / K14 / first K15
    DBuf<int32_t> lord; DBuf<u8> lcnt;
    OrderedLinks L{};
    DBuf<u32> order1;
    bool defer_sorts = false;
    // K17
    DBuf<u64> coff, len64, noff;
    DBuf<u32> clen; DBuf<ExpU> ev;      // the views of expand_repeats (one 32-byte record per unitig); coff / clen: offsets and lengths as plain arrays for what follows
    DBuf<u8> seq_alt, pool, dirty;
    DBuf<u64> shifted;
    u8* cur = nullptr; u8* alt = nullptr;
    u64 final_total = 0;
    bool final_total_pending = false;      // the last rewrite's sum is read with the build's last batch (small outputs: MaterializeFunctor takes it from the device)
    u64 n_links = 0;
    int passes = 0;
    u32 n_cand = 0, n_levels = 0, sparse_sweeps = 0, sparse_start = 0;
    bool partitioned = false;
    DBuf<u8> jowner; DBuf<u32> owned_count, gpre, gpost;
    u32 n_cand_owned = 0;
    DBuf<u32> cpos, prio;
    u64 C = 0;
    DBuf<u32> clist, level;
    DBuf<u32> changed, preds; DBuf<u8> npred;      // changed[9]: the sparse tail's list length, [10..12]: what it reports (MopState::out)
    DBuf<V16> touch;      // the candidate junctions touching each unitig: for the conflict lists here and for every junction that moves something
    DBuf<u64> lkey;
    std::vector<u32> hb;      // first index of every level; [0] = number of levels
    ExpState e{};
    u64 moved_since_rewrite = 0;
    // K15b / K16
    DBuf<u64> seq_words; DBuf<u32> seq_bad;
    DBuf<u32> order2;
    DBuf<u64> number_len, number_len_text, loff;      // (_text: by text-order index, what the path entries are in)
    DBuf<u32> number_only;
    DBuf<u8> meta;
    DBuf<Link> links_out;

    TailRun(GraphBuilder::Impl& impl, FinalGraph* o, bool graph, bool paths) : m(impl), out(o), want_graph(graph), want_paths(paths) {}

    void run() {
        choose_path_export();
        clear_and_write_seqs();
        analyse_and_renumber();
        expand_repeats();
        send_sequences();
        finalise_records();
        finalise_paths();
        collect_and_check();
    }

    void late_copy(std::function<void()> issue) {
        if (late_by_host) late.push_back(LateCopy{side.main_event(), std::move(issue)});
        else { side.after_main(); issue(); }
    }
    void issue_late_copies() { for (auto& c : late) { SideStream::wait_event(c.ev); c.issue(); } late.clear(); }

    // (see PathRemapJob) the entries go now, in seed numbers, under everything that follows
    void choose_path_export() {
        const u64 n_ent = m.n_ent;
        host_remap = want_paths && m.host_remap_allowed && n_ent > 0 &&
                     (host_remap_mode() == 1 || (host_remap_mode() < 0 && n_ent >= (1u << 18) && m.U <= (8u << 20) && path_remap_is_wide()));
        // Round 6: where that table would be too large for the host's caches (more than 8 M unitigs: a mixed-species job) the entries cross as
        // STRETCHES of consecutive text-order numbers (kernels_paths.inc) — 8 bytes per stretch instead of 4 per entry — and the host writes
        // the final numbers out from the table front to back: configs[4]'s 4.8 GB of entries are 84 ms of the 57 GB/s the link gives device ->
        // host (tools/microbench/d2h_probe.hip), behind 3 GB of other late results.  Taken when it at least halves the bytes (one more read-back, on a build of seconds).
        if (!host_remap && want_paths && m.host_remap_allowed && n_ent > 0 && n_ent < 0xFFFFFFF0ULL &&
            (host_remap_mode() == 2 || (host_remap_mode() < 0 && n_ent >= ((u64)1 << 24)))) {
            // (the three mark / rewind pairs stay exactly here: the records outlive the stage, the scratch does not)
            const bool always = host_remap_mode() == 2;
            const Arena::Mark all_mark = Arena::device().mark();
            const u64 rec_cap = always ? n_ent : n_ent / 4 + 1;      // (taken when it at least halves the bytes: at most n_ent / 4 records)
            DBuf<int32_t> rv(rec_cap); DBuf<u32> rp(rec_cap);         // (stay until the build ends: the copies below read them)
            const Arena::Mark scratch_mark = Arena::device().mark();
            const u64 n_groups = (n_ent + 63) / 64;
            DBuf<u32> sflag(n_groups + 1), sat(n_groups + 1);      // (stretch starts per group of 64 entries; [n_groups] = 0: the scan ends with the total)
            launch_full((n_groups + 1) * 64, StretchCountFunctor{m.ent_val.ptr(), n_ent, sflag.ptr()});
            exclusive_scan_u32(sflag.ptr(), sat.ptr(), n_groups + 1);
            n_stretch = read_scalar(sat.ptr() + n_groups);
            if (n_stretch <= rec_cap) {
                launch_full(n_groups * 64, StretchRecordFunctor{m.ent_val.ptr(), n_ent, sat.ptr(), rv.ptr(), rp.ptr()});
                rec_val_block = PinnedPool::get().alloc(n_stretch * 4); rec_pos_block = PinnedPool::get().alloc(n_stretch * 4);
                out->path_block = PinnedPool::get().alloc(n_ent * 4);      // (written by the host's threads, not by a copy)
                side.after_main();
                copy_d2h_async(rec_val_block.p, rv.ptr(), n_stretch * 4, side.stream());
                copy_d2h_async(rec_pos_block.p, rp.ptr(), n_stretch * 4, side.stream());
                host_stretch = true;
            }
            sflag = DBuf<u32>(); sat = DBuf<u32>();
            Arena::device().rewind(host_stretch ? scratch_mark : all_mark);      // (stream 0 reuses the scratch only behind the kernels that read it)
            if (!host_stretch) { rv = DBuf<int32_t>(); rp = DBuf<u32>(); }
        }
        host_numbers = host_remap || host_stretch;      // the device only checks the paths' length sums; the host writes the final numbers
        // (stretch mode: the waves of RemapFunctor — remap_block() entries each — from this one on are the DEVICE's share of the renumbering; see K16 below)
        {
            const u64 n_waves = (n_ent + remap_block() - 1) / remap_block();
            const u32 pct = std::min<u32>(stretch_device_share(), 100u);
            stretch_split_wave = host_stretch ? n_waves - (u64)((double)n_waves * pct / 100.0) : n_waves;
        }
        m.paths_in_seed_numbers = host_numbers;
        if (host_remap) {
            out->path_block = PinnedPool::get().alloc(n_ent * 4);
            side.after_main();
            copy_d2h_async(out->path_block.p, m.ent_val.ptr(), n_ent * 4, side.stream());
        }
    }

    // (both sequence writers: one thread per 64 output bytes; on the device through the block index + LDS tile of seq_write_kernel)
    void write_seqs(int mode, const ExpState* es, const u64* off, u64 n_bytes, u8* dst, bool total_on_device = false) {
        // the indexed / LDS-tiled writer pays for its index (four small launches) from ~16 MB of output on: config C (7.8 MB) 6.02 vs
        // 5.97 ms per build with it, E' (45 MB) 24.9 vs 26.6, config D (126 MB): see DESIGN.md §6
        if (seq_writer_plain() || (n_bytes < ((u64)16 << 20) && !seq_writer_forced())) {
            const u32 per = 16;      // output bytes per thread (r06n: 64 left most of the chip idle on 7.8 MB)
            if (mode == 0) launch((n_bytes + per - 1) / per, SeqFunctor{g.bits.ptr(), off, m.ustartpos.ptr(), m.ulen.ptr(), m.uorient.ptr(), m.U, n_bytes, (int)(m.k / 2), dst, per});
            else launch((n_bytes + per - 1) / per, MaterializeFunctor{*es, off, m.U, n_bytes, dst, per, total_on_device});
            return;
        }
        const u64 n_blocks = (n_bytes + 63) / 64;
        if (n_blocks == 0) return;
        DBuf<u32> bmax(n_blocks), first(n_blocks);
        bmax.fill_bytes(0);
        launch(m.U, BlockMaxFunctor{off, m.U, n_blocks, bmax.ptr()});
        inclusive_max_scan_u32(bmax.ptr(), first.ptr(), n_blocks);
        SeqSrc q{g.bits.ptr(), m.ustartpos.ptr(), m.ulen.ptr(), m.uorient.ptr(), (int)(m.k / 2)};
        ExpState e0{};
        if (mode == 0) launch_wave_kernel(seq_write_kernel<0>, (n_blocks + 255) / 256, 0, q, e0, off, (const u32*)first.ptr(), m.U, n_bytes, dst);
        else launch_wave_kernel(seq_write_kernel<1>, (n_blocks + 255) / 256, 0, q, *es, off, (const u32*)first.ptr(), m.U, n_bytes, dst);
    }

    // K12 sequences
    void clear_and_write_seqs() {
        const u32 U = m.U;
        total = m.N;   // sum of unitig lengths == number of distinct canonical k-mers
        useq.alloc(total);
        // Round 6: every buffer of the tail that starts out cleared — and the scratch of its two renumbering sorts — is allocated HERE, before the
        // tail's first launch, so that their fills leave as one batch with it (a buffer cleared right before its first use cost a fill launch
        // each: fourteen of them between here and the last read-back of a config C build).
        J = (u64)U * 2;
        fixed_start.alloc(U, true); fixed_end.alloc(U, true); cand.alloc((u64)U * 2);
        renum_flag.alloc(1, true); cflag.alloc(J + 1); pool_used.alloc(EXP_SUBPOOLS + 1);
        cflag.fill_bytes(0);       // [J] = 0: the exclusive scan then ends with the total
        pool_used.fill_bytes(0);
        shifted2.alloc(2 * SHIFT_CHECKS); lcount.alloc((u64)U + 1); sums.alloc(n_seqs); n_links_dev.alloc(256);
        shifted2.fill_bytes(0); lcount.fill_bytes(0); sums.fill_bytes(0); n_links_dev.fill_bytes(0);
        if (m.G == &m.loc && !m.loc.h_len.empty()) { u32 mx = 0; for (u32 l : m.loc.h_len) mx = std::max(mx, l); len_bits = 1; while (len_bits < 32 && (mx >> len_bits)) len_bits++; }
        if (!renum_two_pass()) { sort1.prepare(U, 32 + len_bits); sort2.prepare(U, 32 + len_bits); }
        write_seqs(0, nullptr, m.useq_off.ptr(), total, useq.ptr());
        m.lap(&m.tm->seqs);
    }

    // K13 link push order, K14 static analysis for expand_repeats, K15 first renumber_unitigs
    void analyse_and_renumber() {
        const u32 U = m.U;
        lord.alloc((u64)U * 10); lcnt.alloc((u64)U * 2);
        launch_full((u64)U * 2, LinkOrderFunctor{m.links.ptr(), lord.ptr(), lcnt.ptr(), m.counters.ptr() + 5, n_links_dev.ptr()});
        L = OrderedLinks{lord.ptr(), lcnt.ptr()};
        launch(U, FixedSpreadFunctor{m.fs0.ptr(), m.fe0.ptr(), L, fixed_start.ptr(), fixed_end.ptr()});
        launch((u64)U * 2, CandFunctor{L, fixed_start.ptr(), fixed_end.ptr(), cand.ptr()});
        if (m.maybe_dest_valid)      // the walk only collected smallest positions where maybe_dest says so: every real candidate must be covered
            launch((u64)U * 2, CandCoveredFunctor{cand.ptr(), m.maybe_dest.ptr(), m.counters.ptr() + 4});
        order1.alloc(U);
        launch(U, IotaFunctor{order1.ptr()});
        defer_sorts = m.deferred_sort_checks();
        renumber_sort(order1, U, m.ulen.ptr(), m.useq_off.ptr(), useq.ptr(), m.depth.ptr(), defer_sorts ? m.sort_flags.ptr() + 1 : renum_flag.ptr(), defer_sorts, &sort1, len_bits, /*order_is_identity=*/true);
        m.lap(&m.tm->analysis);
    }

    // K17 expand_repeats, level-scheduled (see the kernels)
    void expand_repeats() {
        const u32 U = m.U;
        coff.alloc(U); len64.alloc((u64)U + 1); noff.alloc((u64)U + 1);
        clen.alloc(U); ev.alloc(U);
        seq_alt.alloc(total); pool.alloc(std::min<u64>(8 * total + (1u << 20), 0xFFFFFFF0ULL)); dirty.alloc((u64)U * 2);
        shifted.alloc(1);
        launch(U, ExpInitFunctor{m.useq_off.ptr(), m.ulen.ptr(), cand.ptr(), ev.ptr(), coff.ptr(), clen.ptr(), dirty.ptr()});      // core views = the unitigs, dirty = the candidates (three copies, one launch)
        cur = useq.ptr(); alt = seq_alt.ptr();
        final_total = total;
        partitioned = m.n_owners > 1 && (bool)m.tail_xchg;      // (decided by the driver: the same on every rank)
        cpos.alloc(J + 1); prio.alloc(J);
        launch(J, CandFlagFunctor{order1.ptr(), cand.ptr(), cflag.ptr()});
        exclusive_scan_u32(cflag.ptr(), cpos.ptr(), J + 1);
        {      // (... and the number of links, for the buffers of K16)
            u64 part[256];
            ReadBatch rb; rb.add(&n_cand, cpos.ptr() + J, 4); rb.add(part, n_links_dev.ptr(), sizeof part); rb.run();
            n_links = 0;
            for (u64 v : part) n_links += v;
        }
        if (n_cand == 0) {
            passes = 1;   // the reference's single pass that moves nothing (the same on every rank of a sharded build: nothing to merge)
        } else {
            schedule_levels();
            run_passes();
            if (!partitioned) { if (moved_since_rewrite) rewrite(true); }
            else merge_ranks();
        }
        m.tm->simplify_passes = (u32)passes; m.tm->n_candidates = n_cand; m.tm->n_levels = n_levels;
        m.tm->expand_sparse_sweeps = sparse_sweeps; m.tm->expand_sparse_start = sparse_start;
        m.tm->n_candidates_owned = partitioned && n_cand ? n_cand_owned : n_cand;
        m.lap(&m.tm->expand);
    }

    // The candidate list, the conflicts between the candidates, and their levels: hb[lv] .. hb[lv + 1] of clist are level lv's junctions.
    void schedule_levels() {
        const u32 U = m.U;
        C = n_cand;
        clist.alloc(C); level.alloc(C);
        prio.fill_bytes(0xFF);
        changed.alloc(16); preds.alloc(C * MAX_PREDS); npred.alloc(C);
        changed.fill_bytes(0);      // (the first round of sweeps: cleared with this batch)
        RadixScratch sort_lv;
        sort_lv.prepare(C, 32);
        launch(J, CandListFunctor{order1.ptr(), cflag.ptr(), cpos.ptr(), clist.ptr(), prio.ptr()});
        launch(C, FillU32Functor{level.ptr(), 1u});
        touch.alloc(U);
        launch(U, TouchFunctor{L, cand.ptr(), touch.ptr()});
        launch(C, LevelPredsFunctor{L, cand.ptr(), clist.ptr(), prio.ptr(), C, preds.ptr(), npred.ptr(), touch.ptr()});
        if (partitioned) {      // this rank's share of the junctions: the conflict components it owns
            DBuf<u32> parent(C);
            jowner.alloc(C); owned_count.alloc(1); owned_count.fill_bytes(0);
            launch(C, UfInitFunctor{parent.ptr()});
            launch(C, UfUnionFunctor{preds.ptr(), npred.ptr(), C, parent.ptr()});
            launch(C, UfOwnerFunctor{parent.ptr(), m.n_owners, jowner.ptr()});
            launch_full((J + 63) & ~63ULL, OwnedDirtyFunctor{cand.ptr(), prio.ptr(), jowner.ptr(), m.my_owner, dirty.ptr(), owned_count.ptr(), J});
            gpre.alloc(U, true); gpost.alloc(U, true);
        }
        u32 max_level = 1;
        for (int round = 0;; round++) {   // longest-path levels of the conflict DAG, settled front to back (LevelRelaxFunctor); eight sweeps per host
            if (round) changed.fill_bytes(0);       // check, done when the last of them left no candidate open (a sweep settles one more level)
            for (int it = 0; it < 8; it++)
                launch(C, LevelRelaxFunctor{preds.ptr(), npred.ptr(), C, level.ptr(), changed.ptr() + it, it ? changed.ptr() + it - 1 : nullptr, changed.ptr() + 8});
            const std::vector<u32> hc = to_host(changed, 9);
            max_level = std::max(max_level, hc[8]);
            if (hc[7] == 0) break;
        }
        lkey.alloc(C);
        launch(C, LevelKeyFunctor{level.ptr(), lkey.ptr()});
        int level_bits = 1;
        while (level_bits < 32 && (max_level >> level_bits)) level_bits++;
        sort_pairs_u64_u32(lkey, clist, C, level_bits, 0, 0, &sort_lv);      // (the highest level came back with the convergence flags: one or two digits)
        // first index of every level; [0] = number of levels (levels beyond the table: a second, exact read)
        const u32 LV_TABLE = expand_level_table();
        DBuf<u32> bstart((u64)LV_TABLE + 2);
        launch(C, LevelBoundsFunctor{lkey.ptr(), C, bstart.ptr(), LV_TABLE});
        hb = to_host(bstart, (u64)LV_TABLE + 2);
        n_levels = hb[0];
        if (n_levels > LV_TABLE) {
            DBuf<u32> big((u64)n_levels + 2);
            launch(C, LevelBoundsFunctor{lkey.ptr(), C, big.ptr(), n_levels});
            hb = to_host(big, (u64)n_levels + 2);
        }
        hb.resize((size_t)n_levels + 2);
        hb[n_levels + 1] = (u32)C;
        e = ExpState{cur, ev.ptr(), pool.ptr(), pool_used.ptr(), m.minpos_fwd.ptr(), m.minpos_rev.ptr(), dirty.ptr(), cand.ptr(), L, shifted.ptr(), touch.ptr()};
    }

    // Rewrites the sequences contiguously (gained pieces folded into the core views) and empties the pool.  Once after the
    // last pass — and in between whenever the pool is a quarter full: a side that gains again gets a new piece holding its
    // old one as well, so without this the pool use of a many-pass input grows with the square of the passes.
    void rewrite(bool last) {
        const u32 U = m.U;
        if (partitioned) launch(U, ExpFoldFunctor{e, gpre.ptr(), gpost.ptr()});      // (what the fold makes of the gained pieces: the merge below)
        launch((u64)U + 1, ExpLenFunctor{e, len64.ptr(), U});
        exclusive_scan_u64(len64.ptr(), noff.ptr(), (u64)U + 1);
        // (expand_repeats only ever shortens the total — n >= 2 sources lose what ONE destination gains — so the last total is a bound for
        // this one: the last rewrite of a small output launches over the bound and lets the kernel read the sum, one round trip less)
        const bool defer_total = last && !partitioned && (seq_writer_plain() || (final_total < ((u64)16 << 20) && !seq_writer_forced()));
        if (defer_total) { write_seqs(1, &e, noff.ptr(), final_total, alt, /*total_on_device=*/true); final_total_pending = true; }
        else { final_total = read_scalar(noff.ptr() + U); write_seqs(1, &e, noff.ptr(), final_total, alt); }
        launch(U, ExpResetFunctor{e, noff.ptr(), coff.ptr(), clen.ptr()});
        std::swap(cur, alt);
        e.cur = cur;
        if (!last) pool_used.fill_bytes(0);      // (nothing allocates from the pool after the last rewrite)
        moved_since_rewrite = 0;
    }

    void run_level(u32 lv) {
        const u64 cnt = (u64)(hb[lv + 1] - hb[lv]);
        // sixteen lanes per junction, four junctions per wavefront (expand_wave_kernel; the emulation runs the same kernel in
        // lockstep, wave_rt.hpp).  A thread per junction and 8 / 32 / 64 lanes were measured and retired (r06u/v: G = 16
        // wins from config C to mixed-species graphs)
        if (cnt) launch_wave_kernel(expand_wave_kernel<16>, (cnt * 16 + 255) / 256, 0, e, (const u32*)clist.ptr(), (u64)hb[lv], cnt, (u32)pool.size(), m.counters.ptr() + 7);
    }

    // The passes of expand_repeats, two per host check, until one moves nothing.
    void run_passes() {
        const u32 sparse_max = expand_sparse_max();
        const u32 sub_limit = (u32)(pool.size() / 2 / EXP_SUBPOOLS / 2);      // a region half full (or anything in the overflow half) asks for a rewrite
        for (u32 check = 0;; check++) {   // two passes per host check: if the first moved nothing the second is an (uncounted) no-op
            u64* const sh_words = shifted2.ptr() + 2 * (u64)(check % SHIFT_CHECKS);
            if (check && check % SHIFT_CHECKS == 0) shifted2.fill_bytes(0);      // (the words cleared up front are used up)
            for (int half = 0; half < 2; half++) {
                e.shifted = sh_words + half;
                for (u32 lv = 1; lv <= n_levels; lv++) run_level(lv);
            }
            if (sparse_max) {      // the dirty junctions listed, and — if they are few and the second pass moved something — all remaining passes by one workgroup (kernels_tail.inc)
                launch_full((C + 63) & ~63ULL, MopCompactFunctor{clist.ptr(), lkey.ptr(), dirty.ptr(), (u64*)preds.ptr(), changed.ptr() + 9, C});
                const MopState ms{(u64*)preds.ptr(), changed.ptr() + 9, prio.ptr(), level.ptr(), sh_words, changed.ptr() + 10, sparse_max, expand_sparse_list() ? expand_sparse_list() : 8 * sparse_max, sub_limit, std::min(MOP_BATCH, expand_sparse_batch())};
                launch_wave_kernel_sized(expand_mopup_kernel<0>, 1, MOP_THREADS, 0, e, ms, (u32)pool.size(), m.counters.ptr() + 7);
            }
            u64 sh[2]; u32 used = 0; u32 mop[3] = {0, 0, 0};
            {
                std::vector<u32> pu(EXP_SUBPOOLS + 1);
                ReadBatch rb;
                rb.add(sh, sh_words, 16);
                rb.add(pu.data(), pool_used.ptr(), (EXP_SUBPOOLS + 1) * 4);
                if (sparse_max) rb.add(mop, changed.ptr() + 10, 12);
                rb.run();
                for (u32 q = 0; q < EXP_SUBPOOLS; q++) used = std::max(used, pu[q]);
                if (pu[EXP_SUBPOOLS]) used = 0xFFFFFFFFu;
            }
            moved_since_rewrite += sh[0] + sh[1];
            if (sh[0] == 0) { passes += 1; break; }
            passes += 2;
            if (sh[1] == 0) break;
            if (mop[0]) {      // the one-workgroup tail ran: its sweeps are passes of the reference (the last one of a finished tail moved nothing)
                passes += (int)mop[1];
                sparse_sweeps += mop[1]; sparse_start = mop[2];
                if (mop[0] == 1) break;
            }
            if (used > sub_limit || expand_rewrite_always()) rewrite(false);
        }
    }

    // every rank ran its own junctions: merge what they did to the unitigs, field by field (kernels_tail.inc), and agree on
    // the number of passes (the reference's count is that of the component that needed most)
    void merge_ranks() {
        const u32 U = m.U;
        DBuf<u8> fown((u64)U * 3); DBuf<int32_t> lens3((u64)U * 3 + 1);
        launch(U, FieldOwnerFunctor{L, cand.ptr(), prio.ptr(), jowner.ptr(), m.n_owners, fown.ptr()});
        launch(U, OwnedLensFunctor{e, fown.ptr(), gpre.ptr(), gpost.ptr(), m.my_owner, lens3.ptr()});
        const int32_t neg_passes = -(int32_t)passes;
        copy_h2d(lens3.ptr() + (u64)U * 3, &neg_passes, 4);
        stream_sync();
        m.tail_xchg(lens3.ptr(), (u64)U * 3, 1, 0);
        m.tail_xchg(lens3.ptr() + (u64)U * 3, 1, 1, 1);      // MIN of the negated counts
        launch((u64)U + 1, Lens3SumFunctor{lens3.ptr(), len64.ptr(), U});
        exclusive_scan_u64(len64.ptr(), noff.ptr(), (u64)U + 1);
        int32_t min_neg = 0;
        {
            ReadBatch rb;
            rb.add(&final_total, noff.ptr() + U, 8);
            rb.add(&min_neg, lens3.ptr() + (u64)U * 3, 4);
            rb.add(&n_cand_owned, owned_count.ptr(), 4);
            rb.run();
        }
        passes = -min_neg;
        if (final_total > seq_alt.size()) throw DeviceError("internal error: merged sequences longer than before expand_repeats");
        const u32 per = 16;
        launch((final_total + per - 1) / per, MergeSeqFunctor{e, fown.ptr(), gpre.ptr(), gpost.ptr(), m.my_owner, lens3.ptr(), noff.ptr(), U, final_total, alt, per});
        stream_sync();
        m.tail_xchg(alt, final_total, 0, 0);
        launch(U, ExpResetFunctor{e, noff.ptr(), coff.ptr(), clen.ptr()});
        std::swap(cur, alt);
        e.cur = cur;
    }

    // K15b second renumber_unitigs (graph_simplification.rs:39): a stable sort of the CURRENT order on the new
    // sequences; K16 per-unitig outputs in final order, links in get_links_for_gfa order, paths in final numbers
    // D2H on a second stream, each array as soon as it is final, straight into pinned blocks owned by the result; the
    // paths go in four chunks, each copied while the next is still being renumbered.
    void send_sequences() {
        if (!want_graph) return;
        const u32 U = m.U;
        out->seq_block = PinnedPool::get().alloc(final_total + 64);
        // As 2-bit codes, written out by host threads (SeqExpandJob): a quarter of the bytes over the link — where the sequences are most of what
        // is final this late (one species of long genomes: config D 104 of 142 MB, build 24.9 -> 24.3 ms).  Elsewhere the bytes the host's threads
        // then write slow the device's copies into the same memory down by as much as the link saves (mini-E 55.2 = 55.2 ms, config C 3.70 -> 3.76:
        // profiles/r15o_*), so the codes are taken only when the sequences outweigh the other late results two to one — and are at least 32 MB: on
        // D' at k = 201 (10 MB of sequences) the job's fixed costs were 0.1 ms more than the link saved.
        const u64 other_late = (u64)U * 28 + n_links * sizeof(Link);
        if (seq_codes_transfer() == 2 || (seq_codes_transfer() == 1 && final_total >= ((u64)32 << 20) && final_total > 2 * other_late)) {
            const u64 nw = (final_total + 31) / 32;
            seq_words.alloc(nw); seq_bad.alloc(1); seq_bad.fill_bytes(0);
            launch(nw, SeqPack2Functor{cur, final_total, seq_words.ptr(), seq_bad.ptr()});
            seq_words_block = PinnedPool::get().alloc(nw * 8);
            side.after_main();
            copy_d2h_async(seq_words_block.p, seq_words.ptr(), nw * 8, side.stream());
            seq_job.words = (const u64*)seq_words_block.p; seq_job.out = (u8*)out->seq_block.p; seq_job.total = final_total;
            seq_job.landed = side.mark(); seq_job.side = &side;
#ifndef AC_EMU
            AC_HIP_CHECK(hipGetDevice(&seq_job.dev));
            seq_expand_start(seq_job, 12);
#endif
            seq_as_codes = true;
        } else {
            side.after_main();     // sequences are final since the materialise step: their copy runs under the second renumbering
            copy_d2h_async(out->seq_block.p, cur, final_total, side.stream());
        }
    }

    // The second renumbering, the unitig records and the links in final order.  (The late-copy closures capture this run and plain
    // values only: they are issued by finalise_paths, after this function has returned.)
    void finalise_records() {
        const u32 U = m.U;
        order2.alloc(U);
        copy_d2d(order2.ptr(), order1.ptr(), (size_t)U * 4);
        renumber_sort(order2, U, clen.ptr(), coff.ptr(), cur, m.depth.ptr(), defer_sorts ? m.sort_flags.ptr() + 1 : renum_flag.ptr(), defer_sorts, &sort2, len_bits);
        number_len.alloc(U); number_len_text.alloc(U); loff.alloc((u64)U + 1);
        number_only.alloc(host_numbers ? U : 0);
        meta.alloc((size_t)U * 24);
        u64* d_seq_begin = (u64*)meta.ptr();
        double* d_depth = (double*)(meta.ptr() + (size_t)U * 8);
        u32* d_seq_len = (u32*)(meta.ptr() + (size_t)U * 16);
        u32* d_seed_index = (u32*)(meta.ptr() + (size_t)U * 20);
        out->k = m.k;
        out->n_kmers = 2 * (u64)m.N;
        out->n_unitigs = U;
        late_by_host = late_copies() == 2 || (late_copies() == 1 && final_total + (u64)U * 28 + n_links * sizeof(Link) >= ((u64)256 << 20));
        launch(U, FinalMetaFunctor{order2.ptr(), coff.ptr(), clen.ptr(), m.depth.ptr(), lcnt.ptr(), number_len.ptr(), d_seq_begin, d_depth,
                                   d_seq_len, lcount.ptr(), host_numbers ? number_only.ptr() : nullptr, d_seed_index, m.order.ptr(), number_len_text.ptr(), m.uorient.ptr()});
        if (host_numbers) {      // the number table first: the host threads start on the entries while the rest is still crossing
            number_block = PinnedPool::get().alloc((size_t)U * 4);
            remap_job.path = (int32_t*)out->path_block.p; remap_job.n_ent = m.n_ent;
            if (host_stretch) { remap_job.rec_val = (const int32_t*)rec_val_block.p; remap_job.rec_pos = (const u32*)rec_pos_block.p; remap_job.n_rec = n_stretch; }
            remap_job.number = (const u32*)number_block.p; remap_job.n_unitigs = U;
            remap_job.ent_limit = host_stretch ? (u64)stretch_split_wave * remap_block() : ~0ULL;
            const u32* d_number_only = number_only.ptr();
            const int remap_threads = (int)(host_stretch ? 2 * upload_threads() : upload_threads());      // (writing the stretches out is bound by the host's memory, not by its cores' arithmetic: twice the packing threads — configs[4] writes 4.8 GB)
            late_copy([this, U, d_number_only, remap_threads]() {
                copy_d2h_async(number_block.p, d_number_only, (size_t)U * 4, side.stream());
                remap_job.landed = side.mark(); remap_job.side = &side;
#ifndef AC_EMU
                AC_HIP_CHECK(hipGetDevice(&remap_job.dev));
                path_remap_start(remap_job, remap_threads);
#endif
            });
        }
        if (want_graph) {
            out->meta_block = PinnedPool::get().alloc((size_t)U * 24);
            const u8* d_meta = meta.ptr();
            late_copy([this, U, d_meta]() { copy_d2h_async(out->meta_block.p, d_meta, (size_t)U * 24, side.stream()); });
        }
        exclusive_scan_u64(lcount.ptr(), loff.ptr(), (u64)U + 1);
        links_out.alloc(n_links);      // (n_links: counted by LinkOrderFunctor, read with the candidate count)
        launch(U, LinkOutFunctor{order2.ptr(), L, number_len.ptr(), loff.ptr(), links_out.ptr()});
        if (want_graph) {
            out->links_block = PinnedPool::get().alloc(n_links * sizeof(Link));
            const Link* d_links_out = links_out.ptr();
            late_copy([this, d_links_out]() { copy_d2h_async(out->links_block.p, d_links_out, n_links * sizeof(Link), side.stream()); });
        }
    }

    // The paths in final numbers — or, where the host writes them, only the check of their length sums — and the late copies.
    void finalise_paths() {
        const u64 n_ent = m.n_ent;
        if (host_numbers) {      // the device only checks that every path spells its sequence's length (the sums), it stores nothing ...
            const u64 RB = remap_block();
            const u64 n_waves = (n_ent + RB - 1) / RB;
            const u64 w_split = host_stretch ? std::min<u64>(stretch_split_wave, n_waves) : n_waves;
            if (w_split) launch_full(w_split * 64, RemapFunctor{m.ent_val.ptr(), number_len_text.ptr(), m.path_off.ptr(), n_seqs, n_ent, sums.ptr(), 0, (u32)RB, nullptr, false});
            // ... except for the LAST share of a build that sends its paths as stretches (round 6).  The host's threads can only begin when the
            // number table exists and write configs[4]'s 4.8 GB at ~37 GB/s (a table row fetched per ~10-entry stretch: the host's memory latency,
            // tools/microbench/host_write_probe.hip), which ends ~65 ms AFTER the link has delivered everything else; so the entries behind
            // PathRemapJob::ent_limit are renumbered here and follow the other results over the link, and both ends finish together.
            if (w_split < n_waves) {
                const u64 n_chunks = 4, per_chunk = std::max<u64>((n_waves - w_split + n_chunks - 1) / n_chunks, 64);
                for (u64 w = w_split; w < n_waves; w += per_chunk) {
                    const u64 cnt = std::min<u64>(per_chunk, n_waves - w);
                    launch_full(cnt * 64, RemapFunctor{m.ent_val.ptr(), number_len_text.ptr(), m.path_off.ptr(), n_seqs, n_ent, sums.ptr(), w, (u32)RB, nullptr, true});
                    const u64 b = w * RB, e2 = std::min<u64>((w + cnt) * RB, n_ent);
                    const int32_t* d_ent = m.ent_val.ptr();
                    late_copy([this, d_ent, b, e2]() { copy_d2h_async((int32_t*)out->path_block.p + b, d_ent + b, (e2 - b) * 4, side.stream()); });      // (the one copy stream: behind the unitig records and the links)
                }
            }
        } else {
            if (want_paths) out->path_block = PinnedPool::get().alloc(n_ent * 4);
            const u64 RB = remap_block();
            const u64 n_waves = (n_ent + RB - 1) / RB;
            // Four chunks, each copied while the next is renumbered (the kernel storing straight into the pinned block measured equal, r08j:
            // either way the 4 bytes per entry cross PCIe after the final numbering exists — 42 MB = 0.7 ms on config C)
            // (round 6: from 256 MB of entries on, eight chunks alternating between two copy streams — configs[4] moves 4.8 GB here, and one copy
            // queue alone ran at 33 GB/s)
            const u64 n_chunks = n_ent * 4 >= ((u64)256 << 20) ? 8 : 4;
            const u64 per_chunk = std::max<u64>((n_waves + n_chunks - 1) / n_chunks, 64);
            int turn = 0;
            for (u64 w = 0; w < n_waves; w += per_chunk) {
                u64 cnt = std::min<u64>(per_chunk, n_waves - w);
                launch_full(cnt * 64, RemapFunctor{m.ent_val.ptr(), number_len_text.ptr(), m.path_off.ptr(), n_seqs, n_ent, sums.ptr(), w, (u32)RB, nullptr, true});
                if (want_paths) {
                    u64 b = w * RB, e2 = std::min<u64>((w + cnt) * RB, n_ent);
                    const int which = n_chunks == 8 ? (turn++ & 1) : 0;
                    side.after_main(which);
                    copy_d2h_async((int32_t*)out->path_block.p + b, m.ent_val.ptr() + b, (e2 - b) * 4, side.stream(which));
                }
            }
        }
        issue_late_copies();      // (every kernel of the build is enqueued: from here on this thread only waits)
        m.lap(&m.tm->finalize);
    }

    // The build's last read-back, the host jobs joined, and every consistency check, in their order of precedence.
    void collect_and_check() {
        const u32 U = m.U; const u64 n_ent = m.n_ent;
        PackedText& loc = m.loc;
        std::vector<u64> h_sums(n_seqs);
        out->path_off.resize((size_t)n_seqs + 1);
        std::vector<u32> errs(8);
        u32 pack_bad[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
        u32 h_sort_flags[2] = {0, 0};
        u64 n_links_check = 0, final_total_read = 0; u32 h_seq_bad = 0;
        {
            ReadBatch rb;
            rb.add(h_sums.data(), sums.ptr(), (size_t)n_seqs * 8);
            rb.add(out->path_off.data(), m.path_off.ptr(), ((size_t)n_seqs + 1) * 8);
            rb.add(errs.data(), m.counters.ptr(), 8 * 4);
            rb.add(h_sort_flags, m.sort_flags.ptr(), 8);
            rb.add(&n_links_check, loff.ptr() + U, 8);
            if (final_total_pending) rb.add(&final_total_read, noff.ptr() + U, 8);
            if (loc.check_alphabet && loc.pack_bad.size()) rb.add(pack_bad, loc.pack_bad.ptr(), 8);
            if (seq_as_codes) rb.add(&h_seq_bad, seq_bad.ptr(), 4);
            rb.run();                                   // synchronises stream 0 (once)
        }
        const double t_main_done = now_s();
        side.sync();                                    // ... and the copies: everything above has landed
        const double t_copies_done = now_s();
        if (seq_as_codes) {
#ifdef AC_EMU
            for (u64 b = 0; b < final_total; b += 4096) seq_expand_range(seq_job.words, seq_job.out, b, std::min<u64>(b + 4096, final_total));
#endif
            seq_expand_finish(seq_job);
            if (seq_job.ready.load() == 3) throw DeviceError("internal error: the sequence codes did not reach the host");
            if (h_seq_bad) {      // (never, short of a bug: a byte that is no base in a trimmed unitig sequence — the bytes themselves, then)
                copy_d2h_async(out->seq_block.p, cur, final_total, side.stream());
                side.sync();
            }
        }
        if (host_numbers) {
#ifdef AC_EMU
            if (host_stretch) { for (u64 b = 0; b < n_stretch; b += 7) path_stretch_range(remap_job, b, std::min<u64>(b + 7, n_stretch), &remap_job.bad); }      // (small blocks: the partial lines where two threads' blocks meet)
            else path_remap_range(remap_job.path, n_ent, remap_job.number, U, &remap_job.bad);
#endif
            path_remap_finish(remap_job);
        }
        m.tm->path_stretches = host_stretch ? n_stretch : 0;
        if (knobs().debug_arena && seq_as_codes)
            fprintf(stderr, "d2h: sequence codes: job started %.3f ms before stream 0 drained, its codes had landed %.3f ms after that start, %.1f MB written out in %.3f ms more\n",
                    (t_main_done - seq_job.t_start.load()) * 1e3, (seq_job.t_ready.load() - seq_job.t_start.load()) * 1e3, final_total / 1e6, (seq_job.t_last.load() - seq_job.t_ready.load()) * 1e3);
        if (knobs().debug_arena && host_numbers)
            fprintf(stderr, "d2h: the host's renumbering threads started %.3f ms %s stream 0 drained (their table had landed) and were done %.3f ms later\n",
                    std::fabs(remap_job.t_ready.load() - t_main_done) * 1e3, remap_job.t_ready.load() < t_main_done ? "before" : "after", (remap_job.t_last.load() - remap_job.t_ready.load()) * 1e3);
        if (knobs().debug_arena)      // (where the d2h stage goes: stream 0 drained -> the copies landed -> the host's renumbering threads done)
            fprintf(stderr, "d2h: copies landed %.3f ms after stream 0 drained, host renumbering done %.3f ms later; late results %.1f MB (sequences %.1f, unitig records %.1f, links %.1f, number table %.1f), entries %.1f MB\n",
                    (t_copies_done - t_main_done) * 1e3, (now_s() - t_copies_done) * 1e3, (final_total + (double)U * 24 + n_links * sizeof(Link) + (host_numbers ? (double)U * 4 : 0)) / 1e6,
                    final_total / 1e6, (double)U * 24 / 1e6, n_links * sizeof(Link) / 1e6, host_numbers ? (double)U * 4 / 1e6 : 0.0, n_ent * 4 / 1e6);
        if (loc.pack_bad.size()) loc.verify_alphabet(pack_bad);      // before any internal check: a text with foreign bytes explains them all
        if (errs[7] & 128u) throw NeedExactPositions();      // (before anything else: a repeat of the build settles it)
        if (h_sort_flags[0] || h_sort_flags[1]) {
            if (!m.deferred_sort_checks()) throw DeviceError("internal error: a sort flag was left set by a checked sort");
            throw NeedCheckedSorts();      // (the order the flagged sort left is a permutation, not THE order: everything behind it is void)
        }
        if (errs[7]) throw DeviceError("internal error: expand_repeats pool overflow");
        if (n_links_check != n_links) throw DeviceError("internal error: link counts disagree");
        if (final_total_pending) { if (final_total_read > final_total) throw DeviceError("internal error: expand_repeats lengthened the sequences"); final_total = final_total_read; }
        if (errs[3] || errs[4])
            throw DeviceError("internal error: inconsistent unitig ends (codes " + std::to_string(errs[3]) + "/" + std::to_string(errs[4]) + ")");
        if (remap_job.bad.load()) throw DeviceError("internal error: path entries without a unitig");
        if (want_graph) {
            out->seq_begin = (const u64*)out->meta_block.p;
            out->depth = (const double*)((const u8*)out->meta_block.p + (size_t)U * 8);
            out->seq_len = (const u32*)((const u8*)out->meta_block.p + (size_t)U * 16);
            out->seed_index = (const u32*)((const u8*)out->meta_block.p + (size_t)U * 20);
            out->links = (const Link*)out->links_block.p;
        }
        if (want_paths) out->path = (const int32_t*)out->path_block.p;
        out->n_links = n_links;
        out->n_path = n_ent;
        u64 n_self = errs[5];
        u64 links_one_way = (n_links + n_self) / 2;   // link_count().1 (unitig_graph.rs:478-507): a link and its mirror count
                                                       // once; a link that is its own mirror (a+ -> a-, a- -> a+) counts once
        out->pre = GraphStats{U, links_one_way, total};
        out->post = GraphStats{U, links_one_way, final_total};
        out->simplify_passes = passes;
        // The path of every sequence must spell its full length (unitig_graph.rs:160-174, decompress.rs).
        for (u32 s = 0; s < n_seqs; s++)
            if (h_sums[s] != (u64)loc.h_len[s])
                throw DeviceError("internal error: path length mismatch for sequence " + std::to_string(s + 1));
        m.lap(&m.tm->d2h);
        m.tm->total_device = now_s() - m.t_begin;
        m.tm->launches = rt_counters().launches; m.tm->readbacks = rt_counters().readbacks;
        if (knobs().debug_arena)
            fprintf(stderr, "arena: used %.1f MB (peak %.1f) of %.1f MB (n_text %.1f MB), %.3f s in hipMalloc / hipFree so far\n", Arena::device().total_used() / 1e6,
                    Arena::device().peak() / 1e6, Arena::device().capacity() / 1e6, loc.n_text / 1e6, Arena::device().alloc_seconds());
    }
};

}  // namespace

// K12..K17 + D2H: sequences, link push order, expand_repeats, both renumberings, final numbering.  Needs depth,
// min positions and path ends of ALL sequences (reduced over ranks first in a sharded build).
void GraphBuilder::Impl::tail(FinalGraph* out, bool want_graph, bool want_paths) {
    TailRun run(*this, out, want_graph, want_paths);
    run.run();
}

// The tail's kernels sit in this unit's code object, not in a key width's: device_warmup loads it like those (no junction at all: every
// lane returns at once).
void tail_warm() {
#ifndef AC_EMU
    hipLaunchKernelGGL((expand_wave_kernel<16>), dim3(1), dim3(256), 0, 0, ExpState{}, (const u32*)nullptr, (u64)0, (u64)0, 0u, (u32*)nullptr);
    (void)hipGetLastError();
#endif
}

}  // namespace ac
