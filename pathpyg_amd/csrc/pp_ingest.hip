// pathpyg_amd — ingest of integer temporal edge lists on gfx950: the bytes of a `v<sep>w<sep>t` text file -> three int64 columns.
//
// Reference functions replaced (paths relative to the pathpyG repository root):
//   read_csv_temporal_graph              src/pathpyG/io/pandas.py:511-546   (pandas.read_csv of the file)
//   df_to_temporal_graph                 src/pathpyG/io/pandas.py:318-397   (the three columns it takes from the frame)
//
// Two steps per chunk of the file (a chunk ends at a '\n' or at the end of the file and is smaller than 2^31 bytes):
//   line index : pass 1 flags the first byte of every non-blank line (16 bytes per lane) and counts the flags per workgroup,
//                exclusive_scan (pp_scan.hip) turns the counts into output positions, pass 2 flags again and writes the offsets.
//   parse      : one lane per line; neighbouring lanes read neighbouring lines (about 20 bytes each), every byte read lies before the next
//                line start or the end of the buffer.
// Only files of the exact shape `[0-9]{1,18} sep [0-9]{1,18} sep -?[0-9]{1,18}` per line qualify ('\r' directly before '\n' and blank lines
// are allowed).  Anything else is NOT an error of these kernels: they set a bit of the status word and record the smallest offending byte
// offset; the caller then hands the file to pandas, whose type inference decides what such a file means.
//
// Second half of the file: integer n-gram path files (one walk per line, `node sep node ... [sep weight]`) -> nodes, lengths, weights.
//   read_csv_path_data                   src/pathpyG/io/pandas.py:572-599   (csv.reader of the file, ast.literal_eval of every weight)
//   PathData.append_walks                src/pathpyG/core/path_data.py:126-159
// The same two steps with TOKENS in place of lines (a walk may be thousands of nodes long): a token index, then one lane per token.
#include "pp_internal.h"

namespace pp {

constexpr int kIngestLaneBytes = 16;
constexpr int kIngestTile = kBlock * kIngestLaneBytes;      // 4096 bytes per workgroup
constexpr int kIngestMaxDigits = 18;                        // 10^18 - 1 < 2^63: no overflow check needed while accumulating

struct IngestWs {
    int64_t* result;          // {n_lines, status, smallest offending byte offset (INT64_MAX: none), 0}
    int32_t* block_count;     // [tiles]
    int32_t* block_base;      // [tiles + 1]
    void* scratch;
    size_t scratch_bytes;
    size_t total_bytes;
};

static IngestWs carve_ingest(void* ws, int64_t n_bytes) {
    Arena a(ws, (size_t)-1);
    IngestWs w;
    const int64_t tiles = ceil_div(n_bytes > 0 ? n_bytes : 1, kIngestTile);
    w.result = a.take<int64_t>(4);
    w.block_count = a.take<int32_t>(tiles);
    w.block_base = a.take<int32_t>(tiles + 1);
    w.scratch_bytes = scan_ws_bytes(tiles);
    w.scratch = a.take<char>((int64_t)w.scratch_bytes);
    w.total_bytes = a.used;
    return w;
}

__global__ void k_ingest_init(int64_t* result, int64_t status) {
    result[0] = 0;
    result[1] = status;
    result[2] = INT64_MAX;
    result[3] = 0;
}

__device__ __forceinline__ void ingest_flag(int64_t* result, int64_t bit, int64_t offset) {
    atomicOr((unsigned long long*)&result[1], (unsigned long long)bit);
    atomicMin((long long*)&result[2], (long long)offset);
}

// bit k set: byte base + k is the first byte of a non-blank line.  A line starts at byte 0 and behind every '\n'; it is blank when it is
// empty or holds only a '\r' ("\r\n").  No byte at or past n is read.
__device__ __forceinline__ uint32_t line_start_mask(const uint8_t* __restrict__ buf, int64_t n, int64_t base, bool aligned) {
    if (base >= n) return 0u;
    uint8_t c[kIngestLaneBytes + 2];                       // c[0] = the byte in front of the lane's 16, c[17] = the byte behind them
    c[0] = base > 0 ? buf[base - 1] : (uint8_t)'\n';
    if (aligned && base + kIngestLaneBytes <= n) {
        const uint4 q = *reinterpret_cast<const uint4*>(buf + base);
        const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < kIngestLaneBytes; ++k) c[1 + k] = (uint8_t)(word[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < kIngestLaneBytes; ++k) c[1 + k] = base + k < n ? buf[base + k] : (uint8_t)0;
    }
    c[kIngestLaneBytes + 1] = base + kIngestLaneBytes < n ? buf[base + kIngestLaneBytes] : (uint8_t)0;
    uint32_t mask = 0u;
#pragma unroll
    for (int k = 0; k < kIngestLaneBytes; ++k) {
        const bool blank = c[1 + k] == '\n' || (c[1 + k] == '\r' && c[2 + k] == '\n');
        if (c[k] == '\n' && !blank && base + k < n) mask |= 1u << k;
    }
    return mask;
}

// ---- pass 1: line starts per workgroup ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ingest_count(const uint8_t* __restrict__ buf, int64_t n, int32_t* __restrict__ block_count) {
    __shared__ int32_t part[kWavesPerBlock];
    const int64_t base = (int64_t)blockIdx.x * kIngestTile + (int64_t)threadIdx.x * kIngestLaneBytes;
    int32_t s = __popc(line_start_mask(buf, n, base, ((uintptr_t)buf & 15) == 0));
    s = wave_sum(s);
    if (lane_id() == 0) part[wave_id()] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) t += part[w];
        block_count[blockIdx.x] = t;
    }
}

// ---- pass 2: the offsets, in file order -----------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ingest_offsets(const uint8_t* __restrict__ buf, int64_t n, const int32_t* __restrict__ block_base,
                                                          int32_t* __restrict__ line_start, int64_t line_cap, int64_t* __restrict__ result) {
    __shared__ int32_t scratch[kWavesPerBlock + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {             // (result[0] is the scan's total: written by an earlier kernel of the stream)
        const int64_t lines = result[0];
        if (lines == 0) ingest_flag(result, PP_INGEST_NO_LINES, 0);
        if (lines > line_cap) ingest_flag(result, PP_INGEST_LINE_CAP, 0);
    }
    const int64_t base = (int64_t)blockIdx.x * kIngestTile + (int64_t)threadIdx.x * kIngestLaneBytes;
    uint32_t mask = line_start_mask(buf, n, base, ((uintptr_t)buf & 15) == 0);
    int32_t tot;
    int64_t at = (int64_t)block_base[blockIdx.x] + block_exclusive_sum((int32_t)__popc(mask), scratch, &tot);
    while (mask) {
        const int k = __ffs((int)mask) - 1;
        if (at < line_cap) line_start[at] = (int32_t)(base + k);
        ++at;
        mask &= mask - 1u;
    }
}

// ---- parse: one lane per line -----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ingest_parse(const uint8_t* __restrict__ buf, int64_t n, uint8_t sep,
                                                        const int32_t* __restrict__ line_start, int64_t line_cap, int64_t* __restrict__ result,
                                                        int64_t* __restrict__ v_out, int64_t* __restrict__ w_out, int64_t* __restrict__ t_out) {
    // (both bits are final before this kernel starts: the index step of the same stream sets them)
    if (result[1] & (PP_INGEST_NO_LINES | PP_INGEST_LINE_CAP)) return;
    const int64_t lines = result[0] < line_cap ? result[0] : line_cap;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < lines; i += stride) {
        const int64_t start = line_start[i];
        int64_t end = i + 1 < lines ? (int64_t)line_start[i + 1] : n;      // behind the line's own '\n' only blank lines follow up to `end`
        if (end > n) end = n;
        int64_t field[3] = {0, 0, 0};
        int64_t val = 0, bad_at = -1, bad = 0;
        int nfield = 0, ndig = 0;
        bool neg = false;
        for (int64_t p = start; p < end; ++p) {
            const uint8_t c = buf[p];
            if (c >= '0' && c <= '9') {
                if (ndig == kIngestMaxDigits) { bad = PP_INGEST_TOKEN_LONG; bad_at = p; break; }
                val = val * 10 + (c - '0');
                ++ndig;
            } else if (c == sep) {
                if (ndig == 0) { bad = PP_INGEST_TOKEN_EMPTY; bad_at = p; break; }
                if (nfield == 2) { bad = PP_INGEST_FIELD_COUNT; bad_at = p; break; }
                if (nfield == 0) field[0] = val; else field[1] = val;
                ++nfield;
                val = 0;
                ndig = 0;
            } else if (c == '\n') {
                break;
            } else if (c == '-') {
                if (nfield != 2 || ndig != 0 || neg) { bad = PP_INGEST_MINUS; bad_at = p; break; }
                neg = true;
            } else if (c == '\r') {                        // only directly before '\n'
                if (p + 1 >= end || buf[p + 1] != '\n') { bad = PP_INGEST_BAD_CR; bad_at = p; break; }
            } else {
                bad = PP_INGEST_BAD_BYTE; bad_at = p; break;
            }
        }
        if (!bad) {
            if (nfield != 2) { bad = PP_INGEST_FIELD_COUNT; bad_at = start; }
            else if (ndig == 0) { bad = PP_INGEST_TOKEN_EMPTY; bad_at = start; }
        }
        if (bad) { ingest_flag(result, bad, bad_at); continue; }
        field[2] = neg ? -val : val;
        v_out[i] = field[0];
        w_out[i] = field[1];
        t_out[i] = field[2];
    }
}

static bool ingest_sep_ok(int sep) {
    return sep > 0 && sep < 128 && !(sep >= '0' && sep <= '9') && sep != '-' && sep != '\r' && sep != '\n';
}

// ======================================================================================================================================
// n-gram path files: one walk per line, any number of fields, so the TOKENS are indexed (one lane per line would leave a wave waiting for
// its longest walk).  Same two steps: count / exclusive_scan / fill over 16-byte lanes, then one lane per token.
constexpr int kIngestWeightDigits = 15;                     // 10^15 < 2^53: the digits of a weight and the power of ten are exact doubles

struct IngestTokWs {
    int64_t* result;          // {n_lines, status, smallest offending byte offset (INT64_MAX: none), n_tokens}
    int32_t* line_count;      // [tiles]
    int32_t* line_base;       // [tiles + 1]
    int32_t* token_count;     // [tiles]
    int32_t* token_base;      // [tiles + 1]
    void* scratch;
    size_t scratch_bytes;
    size_t total_bytes;
};

static IngestTokWs carve_ingest_tokens(void* ws, int64_t n_bytes) {
    Arena a(ws, (size_t)-1);
    IngestTokWs w;
    const int64_t tiles = ceil_div(n_bytes > 0 ? n_bytes : 1, kIngestTile);
    w.result = a.take<int64_t>(4);
    w.line_count = a.take<int32_t>(tiles);
    w.line_base = a.take<int32_t>(tiles + 1);
    w.token_count = a.take<int32_t>(tiles);
    w.token_base = a.take<int32_t>(tiles + 1);
    w.scratch_bytes = scan_ws_bytes(tiles);
    w.scratch = a.take<char>((int64_t)w.scratch_bytes);
    w.total_bytes = a.used;
    return w;
}

// bit k set: byte base + k (< n) stands directly behind a separator byte.  No byte at or past n is read.
__device__ __forceinline__ uint32_t behind_sep_mask(const uint8_t* __restrict__ buf, int64_t n, int64_t base, uint8_t sep, bool aligned) {
    if (base >= n) return 0u;
    uint8_t c[kIngestLaneBytes];                           // c[k] = the byte in front of byte base + k
    c[0] = base > 0 ? buf[base - 1] : (uint8_t)'\n';
    if (aligned && base + kIngestLaneBytes <= n) {
        const uint4 q = *reinterpret_cast<const uint4*>(buf + base);
        const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k + 1 < kIngestLaneBytes; ++k) c[1 + k] = (uint8_t)(word[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k + 1 < kIngestLaneBytes; ++k) c[1 + k] = base + k < n ? buf[base + k] : (uint8_t)'\n';
    }
    uint32_t mask = 0u;
#pragma unroll
    for (int k = 0; k < kIngestLaneBytes; ++k)
        if (c[k] == sep && base + k < n) mask |= 1u << k;
    return mask;
}

// ---- pass 1: line starts and token starts per workgroup -------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ingest_tok_count(const uint8_t* __restrict__ buf, int64_t n, uint8_t sep,
                                                            int32_t* __restrict__ line_count, int32_t* __restrict__ token_count) {
    __shared__ int32_t part[2][kWavesPerBlock];
    const int64_t base = (int64_t)blockIdx.x * kIngestTile + (int64_t)threadIdx.x * kIngestLaneBytes;
    const bool aligned = ((uintptr_t)buf & 15) == 0;
    const uint32_t lines = line_start_mask(buf, n, base, aligned);
    const uint32_t tokens = lines | behind_sep_mask(buf, n, base, sep, aligned);
    const int32_t sl = wave_sum((int32_t)__popc(lines)), stk = wave_sum((int32_t)__popc(tokens));
    if (lane_id() == 0) { part[0][wave_id()] = sl; part[1][wave_id()] = stk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) { a += part[0][w]; b += part[1][w]; }
        line_count[blockIdx.x] = a;
        token_count[blockIdx.x] = b;
    }
}

// ---- pass 2: the token offsets, every token's line, every line's first token, in file order -------
__global__ __launch_bounds__(kBlock) void k_ingest_tok_fill(const uint8_t* __restrict__ buf, int64_t n, uint8_t sep,
                                                           const int32_t* __restrict__ line_base, const int32_t* __restrict__ token_base,
                                                           int32_t* __restrict__ token_start, int32_t* __restrict__ token_line, int64_t token_cap,
                                                           int32_t* __restrict__ line_first_token, int64_t line_cap, int64_t* __restrict__ result) {
    __shared__ int32_t scratch[kWavesPerBlock + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {             // (result[0] and result[3] are the scans' totals: written by earlier kernels of the stream)
        const int64_t lines = result[0], tokens = result[3];
        if (lines == 0) ingest_flag(result, PP_INGEST_NO_LINES, 0);
        if (lines > line_cap) ingest_flag(result, PP_INGEST_LINE_CAP, 0);
        if (tokens > token_cap) ingest_flag(result, PP_INGEST_TOKEN_CAP, 0);
        if (lines <= line_cap) line_first_token[lines] = (int32_t)tokens;      // the closing entry (line_first_token has line_cap + 1)
    }
    const int64_t base = (int64_t)blockIdx.x * kIngestTile + (int64_t)threadIdx.x * kIngestLaneBytes;
    const bool aligned = ((uintptr_t)buf & 15) == 0;
    const uint32_t lines = line_start_mask(buf, n, base, aligned);
    uint32_t tokens = lines | behind_sep_mask(buf, n, base, sep, aligned);
    int32_t tot;
    int64_t line_at = (int64_t)line_base[blockIdx.x] + block_exclusive_sum((int32_t)__popc(lines), scratch, &tot);
    int64_t token_at = (int64_t)token_base[blockIdx.x] + block_exclusive_sum((int32_t)__popc(tokens), scratch, &tot);
    while (tokens) {
        const int k = __ffs((int)tokens) - 1;
        if (lines >> k & 1u) {
            if (line_at < line_cap) line_first_token[line_at] = (int32_t)token_at;
            ++line_at;
        }
        if (token_at < token_cap) {
            token_start[token_at] = (int32_t)(base + k);
            token_line[token_at] = (int32_t)(line_at - 1);  // (a separator stands on a non-blank line, whose start lies in front of it)
        }
        ++token_at;
        tokens &= tokens - 1u;
    }
}

// ---- parse: one lane per token ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ingest_tok_parse(const uint8_t* __restrict__ buf, int64_t n, uint8_t sep, int weight,
                                                            const int32_t* __restrict__ token_start, const int32_t* __restrict__ token_line,
                                                            const int32_t* __restrict__ line_first_token, int64_t* __restrict__ result,
                                                            int64_t* __restrict__ nodes, int64_t* __restrict__ lengths, float* __restrict__ weights) {
    // (the three bits are final before this kernel starts: the index step of the same stream sets them)
    if (result[1] & (PP_INGEST_NO_LINES | PP_INGEST_LINE_CAP | PP_INGEST_TOKEN_CAP)) return;
    constexpr double kPow10[kIngestWeightDigits + 1] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
    const int64_t n_lines = result[0], n_tokens = result[3];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n_tokens; t += stride) {
        const int64_t start = token_start[t];
        int64_t end = t + 1 < n_tokens ? (int64_t)token_start[t + 1] : n;      // behind the token's own end only blank lines follow up to `end`
        if (end > n) end = n;
        const int64_t line = token_line[t];
        if (line < 0 || line >= n_lines) { ingest_flag(result, PP_INGEST_FIELD_COUNT, start); continue; }
        int64_t val = 0, bad_at = -1, bad = 0, dot_at = -1;
        int ndig = 0, nfrac = 0;
        bool lead0 = false, last = true;                    // last token of its line: ended by '\r', '\n' or the end of the buffer
        for (int64_t p = start; p < end; ++p) {
            const uint8_t c = buf[p];
            if (c >= '0' && c <= '9') {
                if (ndig == kIngestMaxDigits) { bad = PP_INGEST_TOKEN_LONG; bad_at = p; break; }
                if (ndig == 1 && val == 0 && dot_at < 0) lead0 = true;
                val = val * 10 + (c - '0');
                ++ndig;
                if (dot_at >= 0) ++nfrac;
            } else if (c == sep) {                          // (the next token starts at p + 1 == end; at the end of the buffer nothing does)
                last = false;
                if (p + 1 >= n) { bad = PP_INGEST_TOKEN_EMPTY; bad_at = p; }
                break;
            } else if (c == '\n') {
                break;
            } else if (c == '\r') {                        // only directly before '\n'
                if (p + 1 >= end || buf[p + 1] != '\n') { bad = PP_INGEST_BAD_CR; bad_at = p; }
                break;
            } else if (c == '.') {                         // only in a weight, once, behind a digit: judged when the token's role is known
                if (dot_at >= 0 || ndig == 0) { bad = PP_INGEST_BAD_BYTE; bad_at = p; break; }
                dot_at = p;
            } else {
                bad = PP_INGEST_BAD_BYTE; bad_at = p; break;
            }
        }
        if (!bad && ndig == 0) { bad = PP_INGEST_TOKEN_EMPTY; bad_at = start; }
        const bool is_weight = weight != 0 && last;
        if (!bad) {
            if (is_weight) {
                if (ndig > kIngestWeightDigits || lead0 || (dot_at >= 0 && nfrac == 0)) { bad = PP_INGEST_BAD_WEIGHT; bad_at = start; }
            } else if (dot_at >= 0) {
                bad = PP_INGEST_BAD_BYTE; bad_at = dot_at;
            } else if (lead0) {
                bad = PP_INGEST_LEADING_ZERO; bad_at = start;
            }
        }
        if (!bad && (int64_t)line_first_token[line] == t) {  // the line's first token also answers for the line
            const int64_t fields = (int64_t)line_first_token[line + 1] - t;
            if (weight != 0 && fields < 2) { bad = PP_INGEST_FIELD_COUNT; bad_at = start; }
            else lengths[line] = fields - (weight != 0 ? 1 : 0);
        }
        if (bad) { ingest_flag(result, bad, bad_at); continue; }
        if (is_weight) weights[line] = (float)((double)val / kPow10[nfrac]);   // one correctly rounded division, one rounding to float32
        else nodes[weight != 0 ? t - line : t] = val;
    }
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_ingest_index_ws_bytes(int64_t n_bytes) { return carve_ingest(nullptr, n_bytes).total_bytes; }
size_t pp_ingest_parse_ws_bytes(int64_t n_bytes) { return carve_ingest(nullptr, n_bytes).total_bytes; }      // (the SAME workspace)

int pp_ingest_index(const uint8_t* bytes, int64_t n_bytes, int sep, int32_t* line_start, int64_t line_cap, void* ws, size_t ws_bytes,
                    pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_bytes >= 0 && line_cap >= 0, PP_ERR_ARG, "pp_ingest_index: negative size");
    PP_REQUIRE(n_bytes < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_ingest_index: a chunk of 2^31 bytes or more (%lld)", (long long)n_bytes);
    PP_REQUIRE(ingest_sep_ok(sep), PP_ERR_ARG, "pp_ingest_index: separator %d is not one ASCII byte other than a digit, '-', CR and LF", sep);
    IngestWs w = carve_ingest(ws, n_bytes);
    PP_REQUIRE(ws_bytes >= w.total_bytes, PP_ERR_WORKSPACE, "pp_ingest_index: workspace too small");
    k_ingest_init<<<1, 1, 0, st>>>(w.result, n_bytes == 0 ? (int64_t)PP_INGEST_NO_LINES : 0);
    PP_LAUNCH_CHECK();
    if (n_bytes == 0) return PP_OK;
    const int64_t tiles = ceil_div(n_bytes, kIngestTile);
    k_ingest_count<<<(unsigned)tiles, kBlock, 0, st>>>(bytes, n_bytes, w.block_count);
    PP_LAUNCH_CHECK();
    int rc = exclusive_scan<int32_t, int32_t>(w.block_count, tiles, w.block_base, true, w.result, w.scratch, w.scratch_bytes, st);
    if (rc != PP_OK) return rc;
    k_ingest_offsets<<<(unsigned)tiles, kBlock, 0, st>>>(bytes, n_bytes, w.block_base, line_start, line_cap, w.result);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_ingest_parse(const uint8_t* bytes, int64_t n_bytes, int sep, const int32_t* line_start, int64_t line_cap, int64_t* v, int64_t* w,
                    int64_t* t, void* ws, size_t ws_bytes, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_bytes >= 0 && line_cap >= 0, PP_ERR_ARG, "pp_ingest_parse: negative size");
    PP_REQUIRE(n_bytes < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_ingest_parse: a chunk of 2^31 bytes or more (%lld)", (long long)n_bytes);
    PP_REQUIRE(ingest_sep_ok(sep), PP_ERR_ARG, "pp_ingest_parse: separator %d is not one ASCII byte other than a digit, '-', CR and LF", sep);
    IngestWs ws_ = carve_ingest(ws, n_bytes);
    PP_REQUIRE(ws_bytes >= ws_.total_bytes, PP_ERR_WORKSPACE, "pp_ingest_parse: workspace too small");
    if (n_bytes == 0 || line_cap == 0) return PP_OK;
    int64_t g = ceil_div(line_cap, kBlock);
    if (g > kMaxGrid) g = kMaxGrid;
    k_ingest_parse<<<(unsigned)g, kBlock, 0, st>>>(bytes, n_bytes, (uint8_t)sep, line_start, line_cap, ws_.result, v, w, t);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_ingest_tokens_ws_bytes(int64_t n_bytes) { return carve_ingest_tokens(nullptr, n_bytes).total_bytes; }

int pp_ingest_tokens_index(const uint8_t* bytes, int64_t n_bytes, int sep, int32_t* token_start, int32_t* token_line, int64_t token_cap,
                           int32_t* line_first_token, int64_t line_cap, void* ws, size_t ws_bytes, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_bytes >= 0 && token_cap >= 0 && line_cap >= 0, PP_ERR_ARG, "pp_ingest_tokens_index: negative size");
    PP_REQUIRE(n_bytes < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_ingest_tokens_index: a chunk of 2^31 bytes or more (%lld)", (long long)n_bytes);
    PP_REQUIRE(ingest_sep_ok(sep), PP_ERR_ARG, "pp_ingest_tokens_index: separator %d is not one ASCII byte other than a digit, '-', CR and LF", sep);
    IngestTokWs w = carve_ingest_tokens(ws, n_bytes);
    PP_REQUIRE(ws_bytes >= w.total_bytes, PP_ERR_WORKSPACE, "pp_ingest_tokens_index: workspace too small");
    k_ingest_init<<<1, 1, 0, st>>>(w.result, n_bytes == 0 ? (int64_t)PP_INGEST_NO_LINES : 0);
    PP_LAUNCH_CHECK();
    if (n_bytes == 0) return PP_OK;
    const int64_t tiles = ceil_div(n_bytes, kIngestTile);
    k_ingest_tok_count<<<(unsigned)tiles, kBlock, 0, st>>>(bytes, n_bytes, (uint8_t)sep, w.line_count, w.token_count);
    PP_LAUNCH_CHECK();
    int rc = exclusive_scan<int32_t, int32_t>(w.line_count, tiles, w.line_base, true, w.result, w.scratch, w.scratch_bytes, st);
    if (rc != PP_OK) return rc;
    rc = exclusive_scan<int32_t, int32_t>(w.token_count, tiles, w.token_base, true, w.result + 3, w.scratch, w.scratch_bytes, st);
    if (rc != PP_OK) return rc;
    k_ingest_tok_fill<<<(unsigned)tiles, kBlock, 0, st>>>(bytes, n_bytes, (uint8_t)sep, w.line_base, w.token_base, token_start, token_line,
                                                         token_cap, line_first_token, line_cap, w.result);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_ingest_tokens_parse(const uint8_t* bytes, int64_t n_bytes, int sep, int weight, const int32_t* token_start,
                           const int32_t* token_line, int64_t token_cap, const int32_t* line_first_token, int64_t line_cap,
                           int64_t* nodes, int64_t* lengths, float* weights, void* ws, size_t ws_bytes, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_bytes >= 0 && token_cap >= 0 && line_cap >= 0, PP_ERR_ARG, "pp_ingest_tokens_parse: negative size");
    PP_REQUIRE(n_bytes < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_ingest_tokens_parse: a chunk of 2^31 bytes or more (%lld)", (long long)n_bytes);
    PP_REQUIRE(ingest_sep_ok(sep), PP_ERR_ARG, "pp_ingest_tokens_parse: separator %d is not one ASCII byte other than a digit, '-', CR and LF", sep);
    PP_REQUIRE(weight == 0 || weights != nullptr, PP_ERR_ARG, "pp_ingest_tokens_parse: weight column asked for without a weights buffer");
    IngestTokWs w = carve_ingest_tokens(ws, n_bytes);
    PP_REQUIRE(ws_bytes >= w.total_bytes, PP_ERR_WORKSPACE, "pp_ingest_tokens_parse: workspace too small");
    if (n_bytes == 0 || token_cap == 0 || line_cap == 0) return PP_OK;
    int64_t g = ceil_div(token_cap < n_bytes ? token_cap : n_bytes, kBlock);
    if (g > kMaxGrid) g = kMaxGrid;
    k_ingest_tok_parse<<<(unsigned)g, kBlock, 0, st>>>(bytes, n_bytes, (uint8_t)sep, weight, token_start, token_line, line_first_token, w.result,
                                                      nodes, lengths, weights);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
