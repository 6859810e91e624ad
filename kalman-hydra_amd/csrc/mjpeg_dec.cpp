// Motion-JPEG decoding, host side: the header parser, the marker scan that cuts a frame into restart intervals, the host
// entropy path (mjpeg_dec_core.h's routine on CPU threads) and hm_mjpeg_probe / hm_mjpeg_intervals.  No HIP in this
// file: tools/mjpeg_dec_check.cpp compiles it with the sanitizers as it stands.  Rules: include/hydra_mi.h,
// "Motion-JPEG, decoding"; DESIGN section 23.
#include "mjpeg_dec_core.h"
#include "mjpeg_tables.h"
#include "../../include/hydra_mi.h"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

void hm_set_error(const char *fmt, ...);

#define MJD_REFUSE(...)                  \
    do {                                 \
        hm_set_error(__VA_ARGS__);       \
        return HM_ERR_ARG;               \
    } while (0)

namespace {

// BITS / HUFFVAL -> the decode table.  false: more codes of a length than there are (the table is over-subscribed).
bool mjd_build(const uint8_t bits[16], const uint8_t *vals, int nvals, MjdHuff *h)
{
    memset(h, 0, sizeof(*h));
    memcpy(h->vals, vals, (size_t)nvals);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        h->maxcode[l] = -1;
        h->valoff[l] = k - (int32_t)code;
        for (int i = 0; i < bits[l - 1]; i++, k++, code++) {
            if (code >= (1u << l)) return false;
            if (l <= 8)
                for (uint32_t f = 0; f < (1u << (8 - l)); f++)
                    h->look[(code << (8 - l)) | f] = (uint16_t)((l << 8) | vals[k]);
            h->maxcode[l] = (int32_t)code;
        }
        code <<= 1;
    }
    h->maxcode[0] = -1;
    return true;
}

}  // namespace

int mjd_parse(const uint8_t *b, uint64_t n, MjdParsed *out)
{
    if (!b || !out) MJD_REFUSE("MJPEG: NULL argument");
    if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) MJD_REFUSE("MJPEG: no SOI at the start of the %llu bytes", (unsigned long long)n);
    if (n >= (1ull << 31)) MJD_REFUSE("MJPEG: a frame of %llu bytes, 2^31 or more", (unsigned long long)n);
    MjdParsed &o = *out;
    o.W = o.H = o.components = o.ri = 0;
    o.hs = o.vs = 1;
    o.intervals.clear();                                             // (keeps its capacity: nothing is allocated per frame)
    memset(&o.frame, 0, sizeof(o.frame));
    struct Comp { int id, h, v, tq; } comp[3] = {};
    struct Tab { bool defined = false; MjdHuff h; };
    Tab huff[8];                                                     // [class * 4 + index]
    bool quant_defined[4] = {false, false, false, false};
    uint16_t quant[4][64];
    bool sof = false;
    uint64_t p = 2, scan = 0;
    while (!scan) {
        if (p + 2 > n) MJD_REFUSE("MJPEG: the file ends at byte %llu, before SOS", (unsigned long long)n);
        if (b[p] != 0xFF) MJD_REFUSE("MJPEG: byte %02X at %llu where a marker should be", b[p], (unsigned long long)p);
        if (b[p + 1] == 0xFF) { p++; continue; }                      // fill
        const int m = b[p + 1];
        p += 2;
        if (m == 0xD9) MJD_REFUSE("MJPEG: EOI before SOS");
        if (m == 0x00 || m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7))
            MJD_REFUSE("MJPEG: marker FF%02X before SOS", m);
        if (p + 2 > n) MJD_REFUSE("MJPEG: the file ends inside marker FF%02X", m);
        const uint64_t L = ((uint64_t)b[p] << 8) | b[p + 1];
        if (L < 2 || p + L > n) MJD_REFUSE("MJPEG: segment FF%02X of length %llu does not fit the file", m, (unsigned long long)L);
        const uint8_t *s = b + p + 2;
        const uint64_t sn = L - 2;
        if (m == 0xC0) {
            if (sof) MJD_REFUSE("MJPEG: a second SOF0");
            if (sn < 6) MJD_REFUSE("MJPEG: SOF0 of %llu bytes", (unsigned long long)sn);
            if (s[0] != 8) MJD_REFUSE("MJPEG: sample precision %d, not 8 bits", s[0]);
            o.H = (s[1] << 8) | s[2];
            o.W = (s[3] << 8) | s[4];
            o.components = s[5];
            if (o.W < 1 || o.H < 1) MJD_REFUSE("MJPEG: SOF0 with frame size %dx%d", o.W, o.H);
            if (o.components != 1 && o.components != 3) MJD_REFUSE("MJPEG: %d components, not 1 or 3", o.components);
            if (sn != 6 + 3ull * o.components) MJD_REFUSE("MJPEG: SOF0 of %llu bytes for %d components", (unsigned long long)sn, o.components);
            for (int c = 0; c < o.components; c++) {
                comp[c] = Comp{s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]};
                const bool ok = o.components == 1 ? (comp[c].h >= 1 && comp[c].h <= 4 && comp[c].v >= 1 && comp[c].v <= 4)
                                : c == 0         ? (comp[c].h >= 1 && comp[c].h <= 2 && comp[c].v >= 1 && comp[c].v <= 2)
                                                 : (comp[c].h == 1 && comp[c].v == 1);
                if (!ok) MJD_REFUSE("MJPEG: sampling factors %dx%d of component %d", comp[c].h, comp[c].v, c);
                if (comp[c].tq > 3) MJD_REFUSE("MJPEG: quantisation table %d of component %d", comp[c].tq, c);
            }
            if (o.components == 3) { o.hs = comp[0].h; o.vs = comp[0].v; }    // (one component: an MCU is one block)
            sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            MJD_REFUSE("MJPEG: SOF%d (marker FF%02X): only baseline sequential frames (SOF0) are decoded", m - 0xC0, m);
        } else if (m == 0xCC) {
            MJD_REFUSE("MJPEG: DAC (marker FFCC): arithmetic coding");
        } else if (m == 0xC8) {
            MJD_REFUSE("MJPEG: marker FFC8 (JPG extension)");
        } else if (m == 0xC4) {
            uint64_t i = 0;
            while (i < sn) {
                if (i + 17 > sn) MJD_REFUSE("MJPEG: DHT ends inside a table");
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) MJD_REFUSE("MJPEG: DHT table class %d index %d", tc, th);
                int nv = 0;
                for (int l = 0; l < 16; l++) nv += s[i + 1 + l];
                if (nv > 256 || i + 17 + (uint64_t)nv > sn) MJD_REFUSE("MJPEG: DHT with %d symbols does not fit its segment", nv);
                Tab &t = huff[(size_t)tc * 4 + th];
                if (!mjd_build(s + i + 1, s + i + 17, nv, &t.h)) MJD_REFUSE("MJPEG: DHT class %d index %d has more codes of a length than exist", tc, th);
                t.defined = true;
                i += 17 + (uint64_t)nv;
            }
        } else if (m == 0xDB) {
            uint64_t i = 0;
            while (i < sn) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq != 0) MJD_REFUSE("MJPEG: 16-bit DQT (precision %d of table %d)", pq, tq);
                if (tq > 3 || i + 65 > sn) MJD_REFUSE("MJPEG: DQT table %d does not fit its segment", tq);
                for (int k = 0; k < 64; k++) quant[tq][k] = s[i + 1 + k];
                quant_defined[tq] = true;
                i += 65;
            }
        } else if (m == 0xDD) {
            if (sn != 2) MJD_REFUSE("MJPEG: DRI of %llu bytes", (unsigned long long)sn);
            o.ri = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!sof) MJD_REFUSE("MJPEG: SOS before SOF0");
            if (sn < 1 || sn != 4 + 2ull * s[0]) MJD_REFUSE("MJPEG: SOS of %llu bytes", (unsigned long long)sn);
            if (s[0] != o.components)
                MJD_REFUSE("MJPEG: a scan of %d of the %d components (several scans)", s[0], o.components);
            MjdScan &g = o.frame.scan;
            int slots = 0, slot_of[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
            for (int c = 0; c < o.components; c++) {
                const int id = s[1 + 2 * c], td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (id != comp[c].id) MJD_REFUSE("MJPEG: SOS names component %d where SOF0 has %d", id, comp[c].id);
                if (td > 3 || ta > 3) MJD_REFUSE("MJPEG: SOS names Huffman tables %d / %d", td, ta);
                const int want[2] = {td, 4 + ta};
                for (int w = 0; w < 2; w++) {
                    const int key = want[w], cls = key >> 2, idx = key & 3;
                    if (slot_of[key] < 0) {
                        MjdHuff &h = o.frame.tab[slots];
                        if (huff[(size_t)key].defined) h = huff[(size_t)key].h;
                        else if (idx > 1) MJD_REFUSE("MJPEG: Huffman table class %d index %d is not defined and Annex K has none", cls, idx);
                        else if (cls == 0) (void)mjd_build(MJ_DC_BITS[idx], MJ_DC_VALS, 12, &h);
                        else (void)mjd_build(MJ_AC_BITS[idx], MJ_AC_VALS[idx], 162, &h);
                        slot_of[key] = slots++;
                    }
                    (w ? g.ac_slot : g.dc_slot)[c] = (uint8_t)slot_of[key];
                }
            }
            const uint8_t *e = s + 1 + 2 * o.components;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0)
                MJD_REFUSE("MJPEG: SOS with spectral selection %d..%d, approximation %02X: not a baseline scan", e[0], e[1], e[2]);
            if (!quant_defined[comp[0].tq]) MJD_REFUSE("MJPEG: quantisation table %d is not defined", comp[0].tq);
            memcpy(o.frame.quant, quant[comp[0].tq], sizeof(o.frame.quant));
            g.hs = o.hs; g.vs = o.vs; g.ncomp = o.components;
            g.mw = (o.W + 8 * o.hs - 1) / (8 * o.hs);
            g.mh = (o.H + 8 * o.vs - 1) / (8 * o.vs);
            g.n_mcu = (uint32_t)g.mw * (uint32_t)g.mh;
            g.ri = o.ri ? (uint32_t)o.ri : g.n_mcu;
            scan = p + L;
        }
        // APPn, COM and whatever else carries a length: skipped
        p += L;
    }
    // the entropy-coded segment: markers are FF followed by neither 00 nor FF
    const MjdScan &g = o.frame.scan;
    const uint64_t expect = ((uint64_t)g.n_mcu + g.ri - 1) / g.ri;      // intervals
    uint64_t start = scan, i = scan;
    bool eoi = false;
    while (i + 1 < n) {
        if (b[i] != 0xFF || b[i + 1] == 0x00 || b[i + 1] == 0xFF) { i++; continue; }
        const int m = b[i + 1];
        if (m == 0xD9) { eoi = true; break; }
        if (m == 0xDA) MJD_REFUSE("MJPEG: a second scan (SOS at byte %llu)", (unsigned long long)i);
        if (m < 0xD0 || m > 0xD7) MJD_REFUSE("MJPEG: marker FF%02X at byte %llu inside the scan", m, (unsigned long long)i);
        if (!o.ri) MJD_REFUSE("MJPEG: RST%d at byte %llu of a frame without DRI", m - 0xD0, (unsigned long long)i);
        const uint64_t k = o.intervals.size();
        if (k + 1 >= expect) MJD_REFUSE("MJPEG: more than the %llu RST markers of %u MCUs at DRI %d", (unsigned long long)(expect - 1), g.n_mcu, o.ri);
        if ((uint64_t)(m - 0xD0) != (k & 7)) MJD_REFUSE("MJPEG: RST%d at byte %llu where RST%d is due", m - 0xD0, (unsigned long long)i, (int)(k & 7));
        o.intervals.push_back(MjdInterval{(uint32_t)start, (uint32_t)i, (uint32_t)(k * g.ri)});
        start = i = i + 2;
    }
    const uint64_t end = eoi ? i : n;                                   // (a file cut before EOI: the last interval ends with it)
    const uint64_t k = o.intervals.size();
    if (k + 1 != expect)
        MJD_REFUSE("MJPEG: %llu RST markers, %u MCUs at DRI %d need %llu", (unsigned long long)k, g.n_mcu, o.ri, (unsigned long long)(expect - 1));
    o.intervals.push_back(MjdInterval{(uint32_t)start, (uint32_t)end, (uint32_t)(k * g.ri)});
    o.frame.n_int = (uint32_t)o.intervals.size();
    return HM_OK;
}

uint32_t mjd_entropy_host(const MjdParsed &p, const uint8_t *file, int16_t *coef)
{
    uint32_t bad = 0;
    for (const MjdInterval &iv : p.intervals) bad += (uint32_t)mjd_interval(p.frame.scan, p.frame.tab, file, iv, coef);
    return bad;
}

// ---- the host pool: threads started once, woken for every run ---------------------------------------------------------
struct MjdPool::Impl {
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable wake, done;
    uint64_t generation = 0;
    int active = 0;                                                   // workers that have not finished this generation
    bool quit = false;
    // the job
    int count = 0;
    std::atomic<int> next{0};
    const MjdParsed *const *parsed = nullptr;
    const uint8_t *const *files = nullptr;
    int16_t *const *coef = nullptr;
    uint32_t *bad = nullptr;

    void work()
    {
        for (int i = next++; i < count; i = next++) bad[i] = mjd_entropy_host(*parsed[i], files[i], coef[i]);
    }
    void loop()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            wake.wait(lk, [&] { return quit || generation != seen; });
            if (quit) return;
            seen = generation;
            lk.unlock();
            work();
            lk.lock();
            if (--active == 0) done.notify_one();
        }
    }
};

MjdPool::MjdPool(int threads) : m(new Impl()), n(std::min(std::max(threads, 1), 16))
{
    for (int t = 1; t < n; t++) m->workers.emplace_back([this] { m->loop(); });       // the thread that calls run is one of them
}

MjdPool::~MjdPool()
{
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->quit = true;
    }
    m->wake.notify_all();
    for (std::thread &t : m->workers) t.join();
    delete m;
}

void MjdPool::run(int count, const MjdParsed *const *parsed, const uint8_t *const *files, int16_t *const *coef, uint32_t *bad)
{
    m->count = count; m->parsed = parsed; m->files = files; m->coef = coef; m->bad = bad;
    m->next = 0;
    if (count <= 1 || m->workers.empty()) {                           // nothing to share: nobody is woken
        m->work();
        return;
    }
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->active = (int)m->workers.size();
        m->generation++;
    }
    m->wake.notify_all();
    m->work();
    std::unique_lock<std::mutex> lk(m->mu);
    m->done.wait(lk, [&] { return m->active == 0; });
}

extern "C" int hm_mjpeg_probe(const uint8_t *file, uint64_t n, hm_mjpeg_info *info)
{
    if (!info) MJD_REFUSE("hm_mjpeg_probe: info is NULL");
    MjdParsed p;
    const int rc = mjd_parse(file, n, &p);
    if (rc) return rc;
    info->W = p.W; info->H = p.H; info->components = p.components; info->hs = p.hs; info->vs = p.vs; info->ri = p.ri;
    info->intervals = (uint32_t)p.intervals.size();
    info->mcus = p.frame.scan.n_mcu;
    return HM_OK;
}

extern "C" int hm_mjpeg_intervals(const uint8_t *file, uint64_t n, uint32_t *table, uint64_t cap)
{
    if (!table) MJD_REFUSE("hm_mjpeg_intervals: table is NULL");
    MjdParsed p;
    const int rc = mjd_parse(file, n, &p);
    if (rc) return rc;
    if (cap < p.intervals.size()) MJD_REFUSE("hm_mjpeg_intervals: %zu intervals, room for %llu", p.intervals.size(), (unsigned long long)cap);
    for (size_t i = 0; i < p.intervals.size(); i++) {
        table[3 * i] = p.intervals[i].start; table[3 * i + 1] = p.intervals[i].end; table[3 * i + 2] = p.intervals[i].first_mcu;
    }
    return HM_OK;
}
