// part of net.hip (members of p3d_handle): the fixation pool and shuffled AUC in the evaluation pass (p3d_fixpool_*,
// p3d_eval_shuffled_*, p3d_video_shuffled_begin; fixpool.hip).  Nothing exists before p3d_fixpool_open, and while no
// p3d_eval_shuffled_draws has armed it an evaluation issues what it always issued.  No step, launch list or captured graph names
// the pool.  The host keeps which slots are filled.  The evaluation's part (select, clean moments, borji) is issued by eval_maps
// (net_readout.inc).
    // the union, counts and scan of B rows of M pool slots; its buffers only grow
    struct FixUnion {
        int B = 0, M = 0, n = 0; size_t room = 0; bool begun = false;
        DevMem<unsigned long long> uni; DevMem<unsigned> prefix, bsum, n_other_dev, counter; DevMem<int> ids;
        std::vector<unsigned> n_other;
    };
    // the pool (one bit per pixel and slot), its staging buffer and the two unions.  p3d_fixpool_close assigns a fresh one
    struct FixPool {
        bool is_open = false;
        int H = 0, W = 0;
        int64_t cap = 0, nw = 0;
        DevMem<unsigned long long> words;
        std::vector<char> filled;
        DevMem<unsigned char> staging;      // only grows
        // sh: one batch's union (p3d_eval_shuffled_begin), and the draws that arm the next evaluation
        // vu: the union p3d_video_shuffled_begin holds for p3d_video_score_auc: n frames' rows, in buffers of its own -- sh, armed
        // or not, is neither read nor written
        FixUnion sh, vu;
        bool armed = false, have = false;
        std::vector<int> ranks, n_rows;
        int n_rep = 0; double step = 0.1;
        std::vector<double> last;
        void need_open(const char* what) const {
            if (!is_open) throw P3dError(std::string(what) + ": no fixation pool is open (p3d_fixpool_open)");
        }
        // ids [B][M]: every id a filled slot; 1 <= M <= 64
        void check_ids(const char* what, const int* ids, int B, int M) const {
            need_open(what);
            if (!ids) throw P3dError("null argument");
            if (M < 1 || M > 64) throw P3dError(std::string(what) + ": 1 .. 64 other maps per clip, not " + std::to_string(M));
            for (int b = 0; b < B; ++b)
                for (int m = 0; m < M; ++m) {
                    const int id = ids[(size_t)b * M + m];
                    if (id < 0 || id >= cap) throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": slot " + std::to_string(id) + " is outside [0, " + std::to_string(cap) + ")");
                    if (!filled[(size_t)id]) throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": slot " + std::to_string(id) + " was never filled (p3d_fixpool_put)");
                }
        }
        // ranks [sum n_rows[b]][n_rep]: refused before anything is kept when a row count or a rank exceeds the clip's n_other
        static void check_draws(const char* what, const int* ranks, const int* n_rows, const unsigned* n_other, int B, int n_rep, double step) {
            if (!n_rows) throw P3dError("null argument");
            if (n_rep < 1 || !(step > 0.0)) throw P3dError(std::string(what) + ": n_rep >= 1 and a positive step");
            size_t at = 0;
            for (int b = 0; b < B; ++b) {
                if (n_rows[b] < 0 || (unsigned)n_rows[b] > n_other[b])
                    throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": " + std::to_string(n_rows[b]) + " rows, but the union holds " + std::to_string(n_other[b]) + " fixations");
                const size_t n = (size_t)n_rows[b] * n_rep;
                if (n > 0 && !ranks) throw P3dError("null argument");
                for (size_t i = 0; i < n; ++i)
                    if (ranks[at + i] < 0 || (unsigned)ranks[at + i] >= n_other[b])
                        throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": rank " + std::to_string(ranks[at + i]) + " is outside [0, " + std::to_string(n_other[b]) + ")");
                at += n;
                if (at > (size_t)INT32_MAX) throw P3dError(std::string(what) + ": too many ranks");
            }
        }
    } fixpool;
    // HIP events: last put's packs; last begin; last armed evaluation's select, moments + borji.  They outlive the pool:
    // p3d_fixpool_last_ms asks for no open one
    double fixpool_ms[4] = {0.0, 0.0, 0.0, 0.0};
    void fixpool_open(int H, int W, int64_t capacity) {
        if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("fixpool: maps are H x W bytes, 1 <= H * W <= 2^30");
        if (capacity < 1 || capacity > INT32_MAX) throw P3dError("fixpool: a capacity of 1 .. 2^31 - 1 maps");
        FixPool np;                            // the new pool first: a failure changes nothing
        np.nw = p3d_fix_words((long long)H * W);
        np.words = DevMem<unsigned long long>((size_t)capacity * np.nw, "fixpool_open: no device memory for " + std::to_string(capacity) + " maps");
        np.is_open = true; np.H = H; np.W = W; np.cap = capacity;
        np.filled.assign((size_t)capacity, 0);
        fixpool = std::move(np);
    }
    // maps [n][H][W] from the host into slots first .. first + n - 1, in uploads of at most 256 MB
    void fixpool_put(int64_t first, const unsigned char* maps, int64_t n) {
        fixpool.need_open("fixpool_put");
        if (!maps) throw P3dError("null argument");
        if (n < 1 || first < 0 || first > fixpool.cap - n)
            throw P3dError("fixpool_put: slots " + std::to_string(first) + " .. " + std::to_string(first + n - 1) + " are not inside [0, " + std::to_string(fixpool.cap) + ")");
        const size_t N = (size_t)fixpool.H * fixpool.W;
        const int64_t per = std::min<int64_t>(65535, std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / N)));
        fixpool.staging.grow((size_t)std::min(n, per) * N, "fixpool_put: no device memory for the staging buffer");      // (every earlier call ended synchronised)
        StageTimer tm(true, 2);
        double ms = 0.0;
        for (int64_t done = 0; done < n; done += per) {
            const int64_t cn = std::min(per, n - done);
            FixPackArgs a;
            a.maps = fixpool.staging; a.n = cn; a.n_pix = (long long)N; a.words = fixpool.words + (first + done) * fixpool.nw;
            HIPCHECK(copy_now(fixpool.staging, maps + (size_t)done * N, (size_t)cn * N, hipMemcpyHostToDevice, stream));
            tm.mark(0, stream);
            HIPCHECK(p3d_fix_pack_launch(a, stream));
            tm.mark(1, stream);
            HIPCHECK(hipStreamSynchronize(stream));
            ms += tm.ms(0);
            std::fill(fixpool.filled.begin() + (first + done), fixpool.filled.begin() + (first + done + cn), 1);
        }
        fixpool_ms[0] = ms;
    }
    // The union of B rows of M slots into u's buffers, one launch between tm's marks and the one synchronisation; u.n_other [B].
    // Buffers that are too small go before their successors come: a failure leaves a union that holds nothing.
    void union_issue(FixUnion& u, const int* ids, int B, int M, StageTimer& tm) {
        u.begun = false;
        const int nsb = p3d_fix_scan_blocks(fixpool.nw);
        const size_t room = (size_t)B * fixpool.nw;
        if (room > u.room || B > u.B || M > u.M) {
            const int nB = std::max(B, u.B), nM = std::max(M, u.M);
            const size_t nroom = std::max(room, u.room);
            const char* what = "shuffled_begin: no device memory for the union";
            u = FixUnion();
            if (&u == &fixpool.sh) fixpool.have = false;      // the evaluation's results went with the union they came from
            u.uni = DevMem<unsigned long long>(nroom, what);
            u.prefix = DevMem<unsigned>(nroom, what);
            u.bsum = DevMem<unsigned>((size_t)nB * nsb, what);
            u.n_other_dev = DevMem<unsigned>((size_t)nB, what);
            u.counter = DevMem<unsigned>((size_t)nB, what);
            u.ids = DevMem<int>((size_t)nB * nM, what);
            HIPCHECK(fill_now(u.counter, 0, (size_t)nB * sizeof(unsigned), stream));
            u.room = nroom; u.B = nB; u.M = nM;
        }
        HIPCHECK(copy_now(u.ids, ids, (size_t)B * M * sizeof(int), hipMemcpyHostToDevice, stream));
        FixUnionArgs a;
        a.pool = fixpool.words; a.nw = fixpool.nw; a.ids = u.ids; a.B = B; a.M = M; a.nsb = nsb;
        a.uni = u.uni; a.prefix = u.prefix; a.bsum = u.bsum; a.n_other = u.n_other_dev; a.counter = u.counter;
        tm.mark(0, stream);
        HIPCHECK(p3d_fix_union_launch(a, stream));
        tm.mark(1, stream);
        u.n_other.assign((size_t)B, 0u);
        HIPCHECK(copy_now(u.n_other.data(), u.n_other_dev, (size_t)B * sizeof(unsigned), hipMemcpyDeviceToHost, stream));      // the one synchronisation
        u.n = B; u.begun = true;
    }
    void shuffled_begin(const int* ids, int B, int M, uint32_t* n_other_out) {
        if (!n_other_out) throw P3dError("null argument");
        fixpool.check_ids("eval_shuffled_begin", ids, B, M);
        fixpool.armed = false;
        StageTimer tm(true, 2);
        union_issue(fixpool.sh, ids, B, M, tm);
        fixpool_ms[1] = tm.ms(0);
        std::copy(fixpool.sh.n_other.begin(), fixpool.sh.n_other.end(), n_other_out);
    }
    void shuffled_draws(const int* ranks, const int* n_rows, int n_rep, double step) {
        fixpool.need_open("eval_shuffled_draws");
        if (!fixpool.sh.begun) throw P3dError("eval_shuffled_draws: no union is held (p3d_eval_shuffled_begin)");
        const int B = (int)fixpool.sh.n_other.size();
        fixpool.armed = false;
        FixPool::check_draws("eval_shuffled_draws", ranks, n_rows, fixpool.sh.n_other.data(), B, n_rep, step);
        size_t n = 0;
        for (int b = 0; b < B; ++b) n += (size_t)n_rows[b] * n_rep;
        fixpool.ranks.assign(ranks, ranks + n);
        fixpool.n_rows.assign(n_rows, n_rows + B);
        fixpool.n_rep = n_rep; fixpool.step = step; fixpool.armed = true;
    }
    void video_shuffled_begin(const int* ids, int n, int M, uint32_t* n_other_out) {
        if (!n_other_out) throw P3dError("null argument");
        if (n < 1 || n > 65535) throw P3dError("video_shuffled_begin: 1 .. 65535 frames");
        fixpool.check_ids("video_shuffled_begin", ids, n, M);
        StageTimer tm;      // (not timed)
        union_issue(fixpool.vu, ids, n, M, tm);
        std::copy(fixpool.vu.n_other.begin(), fixpool.vu.n_other.end(), n_other_out);
    }
