// Engine: weights in kernel-optimal layouts, per-sequence KV caches (K rows + Vᵀ columns), prefill / decode
// orchestration, device-resident decode loop, RCCL all-reduce for the tensor-parallel decoder.
//
// Reference call stacks this replaces: llava/model/llava_arch.py:94-97 (encode_images),
// llava/model/language_model/llava_llama.py:88-99 -> HF5:models/llama/modeling_llama.py:367-494 (decoder forward),
// HF5:models/clip/modeling_clip.py:594-657 (CLIP vision transformer).
#include "engine.h"

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace lmx {

thread_local KernelTimer* g_kernel_timer = nullptr;


static thread_local std::string g_err;
void set_last_error(const std::string& s) { g_err = s; }
const char* get_last_error() { return g_err.c_str(); }

#define LMX_CHECK_NCCL(expr)                                                                                 \
    do {                                                                                                     \
        ncclResult_t _r = (expr);                                                                            \
        if (_r != ncclSuccess) throw Error{std::string(#expr) + " failed: " + ncclGetErrorString(_r)};      \
    } while (0)

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

void zero_fill(void* p, size_t n) {
    static std::mutex mu;
    static hipStream_t util = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!util) LMX_CHECK_HIP(hipStreamCreateWithFlags(&util, hipStreamNonBlocking));
    LMX_CHECK_HIP(hipMemsetAsync(p, 0, n, util));
    LMX_CHECK_HIP(hipStreamSynchronize(util));
}

// ---------------------------------------------------------------------------------------------------------------
Model::Model(const lmx_config& c) : cfg(c) {
    LMX_REQUIRE(c.abi_version == LMX_ABI_VERSION, "lmx_config.abi_version mismatch");
    LMX_REQUIRE(c.dtype == kF32 || c.dtype == kBF16 || c.dtype == kF16, "bad dtype");
    LMX_REQUIRE(c.tp_world >= 1 && c.tp_rank >= 0 && c.tp_rank < c.tp_world, "bad tensor-parallel rank/world");
    es = (int)dtype_size(c.dtype);
    // defaults of the options lmx_model_set_option can flip later (A/B runs and the bit-identity tests of the fused forms)
    { const char* e = getenv("LMX_FUSE_ROPE"); if (e) opt_fuse_rope = atoi(e) != 0; }
    { const char* e = getenv("LMX_VIS_PACK"); if (e) opt_vis_pack = atoi(e) != 0; }
    { const char* e = getenv("LMX_DECODE_SPLITQ"); if (e) opt_splitq = atoi(e) != 0; }
    { const char* e = getenv("LMX_DECODE_ROT"); if (e) opt_rot = atoi(e) != 0; }
    if (c.dtype == kF32) opt_rot = false;                     // the hand-counted stream is the 16-bit models'
    { const char* e = getenv("LMX_TP_OVERLAP"); if (e) { tp_overlap = atoi(e) != 0; tp_overlap_force = atoi(e) == 2; } }
    H = c.hidden_size; D = c.head_dim; V = c.vocab_size; Vr = V; L = c.n_layers;
    LMX_REQUIRE(D == 64 || D == 128, "head_dim must be 64 or 128");
    LMX_REQUIRE(c.n_heads % c.tp_world == 0 && c.n_kv_heads % c.tp_world == 0, "heads must divide by tp_world");
    LMX_REQUIRE(c.n_heads % c.n_kv_heads == 0, "n_heads must be a multiple of n_kv_heads");
    LMX_REQUIRE(c.intermediate_size % (32 * c.tp_world) == 0, "intermediate_size must divide by 32*tp_world");
    LMX_REQUIRE(H % 64 == 0, "hidden size must be a multiple of 64");
    LMX_REQUIRE(V % 8 == 0, "vocab_size must be a multiple of 8");
    nh_l = c.n_heads / c.tp_world; nkv_l = c.n_kv_heads / c.tp_world;
    // local MLP width: the rank's I/world columns, zero-padded up to a multiple of 64 so the down-projection's K keeps the GEMM's
    // k-slab granularity (7B at TP=8: 1376 -> 1408).  Padded gate|up rows are zero => silu(0)*0 = 0 => no contribution.
    I_sh = c.intermediate_size / c.tp_world; I_l = round_up(I_sh, 64);
    qkv_n = (nh_l + 2 * nkv_l) * D;
    // vocabulary-parallel lm_head: each rank streams V / world rows per token instead of all of them (262 MB at 7B: 8 % of
    // a TP=1 token, 40 % of a TP=8 token if replicated); replicated when the vocabulary does not split into 8-row-aligned shards
    if (c.tp_world > 1 && V % (8 * c.tp_world) == 0) { V_l = V / c.tp_world; v_off = c.tp_rank * V_l; } else { V_l = V; v_off = 0; }
    s_max = round_up(c.max_position > 0 ? c.max_position : 2048, 128);   // decode attention works in 128-key chunks
    dec.resize(L);

    if (c.v_layers > 0) {
        Dv = c.v_hidden; Fv = c.v_intermediate;
        LMX_REQUIRE(c.v_image_size % c.v_patch_size == 0, "image size must be a multiple of the patch size");
        LMX_REQUIRE(Dv % 64 == 0 && Fv % 64 == 0 && Dv % c.v_heads == 0, "vision widths must be multiples of 64");
        vD = Dv / c.v_heads;
        LMX_REQUIRE(vD == 64 || vD == 128, "vision head_dim must be 64 or 128");
        const int g = c.v_image_size / c.v_patch_size;
        P = g * g; Tv = P + 1;
        kpad = round_up(3 * c.v_patch_size * c.v_patch_size, 64);
        spad = round_up(Tv, 64);
        const int n_hs = c.v_layers + 1;
        int idx = c.select_layer < 0 ? n_hs + c.select_layer : c.select_layer;
        LMX_REQUIRE(idx >= 0 && idx < n_hs, "select_layer out of range");
        v_run = idx;
        vis.resize(v_run);
        out_tokens = c.select_feature == LMX_FEATURE_PATCH ? P : Tv;
        const int nlin = c.projector_type == LMX_PROJ_LINEAR ? 1 : c.projector_type == LMX_PROJ_MLP_GELU ? c.projector_depth : 0;
        LMX_REQUIRE(c.projector_type != LMX_PROJ_MLP_GELU || c.projector_depth >= 1, "mlpNx_gelu needs depth >= 1");
        if (c.projector_type == LMX_PROJ_IDENTITY) LMX_REQUIRE(Dv == H, "identity projector needs mm_hidden_size == hidden_size");
        proj_w.assign(nlin, nullptr); proj_b.assign(nlin, nullptr);
    }
    LMX_CHECK_HIP(hipEventCreateWithFlags(&vws_done, hipEventDisableTiming));
}

Model::~Model() {
    if (comm) (void)ncclCommDestroy(comm);
    for (int r = 0; r < P2P_MAX_WORLD; ++r) if (p2p_peer[r] && p2p_peer[r] != p2p_local) (void)hipIpcCloseMemHandle(p2p_peer[r]);
    if (p2p_local) (void)hipFree(p2p_local);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    for (auto& r : prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto e : prof_pool) (void)hipEventDestroy(e);
    if (vws_done) (void)hipEventDestroy(vws_done);
    if (rope) (void)hipFree(rope);
}

hipEvent_t Model::prof_event() {
    if (!prof_pool.empty()) { hipEvent_t e = prof_pool.back(); prof_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    LMX_CHECK_HIP(hipEventCreate(&e));
    return e;
}

std::map<std::string, Model::ProfAcc> Model::prof_resolve() {
    LMX_CHECK_HIP(hipDeviceSynchronize());
    std::map<std::string, ProfAcc> out;
    for (auto& r : prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { auto& a = out[r.name]; a.ms += ms; a.count += 1; }
        prof_pool.push_back(r.e0); prof_pool.push_back(r.e1);
    }
    prof_recs.clear();
    return out;
}

void* Model::alloc_weight(size_t bytes, bool zero) {
    pool.emplace_back();
    pool.back().ensure(bytes, zero);
    return pool.back().p;
}

static bool starts_with(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }

// copy a [rows x cols] sub-block (row0.., col0..) of a row-major [R x C] matrix into dst (row-major, pitch dst_cols)
static void copy_block(void* dst, int dst_cols, int dst_row0, const void* src, int C, int row0, int col0, int rows, int cols, int es, hipStream_t st) {
    LMX_CHECK_HIP(hipMemcpy2DAsync(static_cast<char*>(dst) + (size_t)dst_row0 * dst_cols * es, (size_t)dst_cols * es,
                                   static_cast<const char*>(src) + ((size_t)row0 * C + col0) * es, (size_t)C * es,
                                   (size_t)cols * es, rows, hipMemcpyDeviceToDevice, st));
}

void Model::load_weight(const std::string& name, const void* src, int dtype, int ndim, const int64_t* shape, hipStream_t st) {
    LMX_REQUIRE(dtype == cfg.dtype, "weight dtype must equal the model dtype (cast on the host side): " + name);
    LMX_REQUIRE(src != nullptr && ndim >= 1 && ndim <= 4, "bad tensor: " + name);
    int64_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= shape[i];
    auto expect = [&](std::initializer_list<int64_t> want) {
        bool ok = (int)want.size() == ndim;
        int i = 0;
        for (auto w : want) { if (ok && shape[i] != w) ok = false; ++i; }
        if (!ok) {
            std::string got = "[", exp = "[";
            for (int k = 0; k < ndim; ++k) got += std::to_string(shape[k]) + (k + 1 < ndim ? "," : "");
            for (auto w : want) exp += std::to_string(w) + ",";
            throw Error{"shape mismatch for " + name + ": got " + got + "] expected " + exp + "]"};
        }
    };
    auto plain = [&](void*& dst) {
        if (!dst) dst = alloc_weight((size_t)numel * es);
        LMX_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)numel * es, hipMemcpyDeviceToDevice, st));
    };
    const int r = cfg.tp_rank;
    const int nh = cfg.n_heads, nkv = cfg.n_kv_heads, I = cfg.intermediate_size;

    if (name == "model.embed_tokens.weight") { expect({V, H}); plain(embed); }
    else if (name == "model.norm.weight") { expect({H}); plain(final_norm); pack_rot_head(st); }      // (the head's launch fuses it: see input_layernorm below)
    else if (name == "lm_head.weight") {
        expect({V, H});
        if (V_l == V) plain(lm_head);
        else {
            if (!lm_head) lm_head = alloc_weight((size_t)V_l * H * es);
            LMX_CHECK_HIP(hipMemcpyAsync(lm_head, static_cast<const char*>(src) + (size_t)v_off * H * es, (size_t)V_l * H * es, hipMemcpyDeviceToDevice, st));
        }
        pack_rot_head(st);                                    // a reload behind finalize(): the rotated copy follows its source
    }
    else if (starts_with(name, "model.layers.")) {
        const size_t p0 = strlen("model.layers.");
        const size_t dot = name.find('.', p0);
        LMX_REQUIRE(dot != std::string::npos, "bad layer name " + name);
        const int li = atoi(name.substr(p0, dot - p0).c_str());
        LMX_REQUIRE(li >= 0 && li < L, "layer index out of range: " + name);
        const std::string sub = name.substr(dot + 1);
        DecLayerW& w = dec[li];
        if (!w.wqkv) {
            auto bytes = [&](DecSite site) { const DecLinear d = dec_linear(site, &w); return (size_t)d.N * d.K * es; };
            w.wqkv = alloc_weight(bytes(DecSite::QKV));
            w.wo = alloc_weight(bytes(DecSite::O));
            w.wgu = alloc_weight(bytes(DecSite::GateUp), I_l != I_sh);
            w.wd = alloc_weight(bytes(DecSite::Down), I_l != I_sh);
        }
        if (sub == "self_attn.q_proj.weight") { expect({(int64_t)nh * D, H}); copy_block(w.wqkv, H, 0, src, H, r * nh_l * D, 0, nh_l * D, H, es, st); pack_rot_layer(w, kRotQ, st); }
        else if (sub == "self_attn.k_proj.weight") { expect({(int64_t)nkv * D, H}); copy_block(w.wqkv, H, nh_l * D, src, H, r * nkv_l * D, 0, nkv_l * D, H, es, st); pack_rot_layer(w, kRotKv, st); }
        else if (sub == "self_attn.v_proj.weight") { expect({(int64_t)nkv * D, H}); copy_block(w.wqkv, H, (nh_l + nkv_l) * D, src, H, r * nkv_l * D, 0, nkv_l * D, H, es, st); pack_rot_layer(w, kRotKv, st); }
        else if (sub == "self_attn.o_proj.weight") { expect({H, (int64_t)nh * D}); copy_block(w.wo, nh_l * D, 0, src, nh * D, 0, r * nh_l * D, H, nh_l * D, es, st); pack_rot_layer(w, kRotO, st); }
        else if (sub == "mlp.gate_proj.weight") { expect({I, H}); launch_interleave_half(cfg.dtype, static_cast<const char*>(src) + (size_t)r * I_sh * H * es, w.wgu, I_sh, H, 0, st); }
        else if (sub == "mlp.up_proj.weight") { expect({I, H}); launch_interleave_half(cfg.dtype, static_cast<const char*>(src) + (size_t)r * I_sh * H * es, w.wgu, I_sh, H, 1, st); }
        else if (sub == "mlp.down_proj.weight") { expect({H, I}); copy_block(w.wd, I_l, 0, src, I, 0, r * I_sh, H, I_sh, es, st); pack_rot_layer(w, kRotDown, st); }
        // the q launch fuses this norm, and whether a launch fuses one is part of what decides its rows per wave: a q copy packed before the norm arrived follows now
        else if (sub == "input_layernorm.weight") { expect({H}); plain(w.ln1); pack_rot_layer(w, kRotQ, st); }
        else if (sub == "post_attention_layernorm.weight") { expect({H}); plain(w.ln2); }
        else if (sub == "self_attn.rotary_emb.inv_freq") { return; }   // buffer in old checkpoints; recomputed
        else throw Error{"unknown decoder tensor: " + name};
    }
    else if (starts_with(name, "mm_projector.")) {
        LMX_REQUIRE(!proj_w.empty(), "projector tensor given but projector is identity/absent: " + name);
        int li = 0; std::string leaf;
        const std::string rest = name.substr(strlen("mm_projector."));
        if (rest == "weight" || rest == "bias") { li = 0; leaf = rest; }
        else {
            const size_t dot = rest.find('.');
            LMX_REQUIRE(dot != std::string::npos, "bad projector name " + name);
            const int seq_idx = atoi(rest.substr(0, dot).c_str());
            LMX_REQUIRE(seq_idx % 2 == 0, "projector index must address a Linear (even index): " + name);
            li = seq_idx / 2; leaf = rest.substr(dot + 1);
        }
        LMX_REQUIRE(li >= 0 && li < (int)proj_w.size(), "projector layer out of range: " + name);
        const int in = li == 0 ? Dv : H;
        if (leaf == "weight") { expect({H, in}); plain(proj_w[li]); }
        else if (leaf == "bias") { expect({H}); plain(proj_b[li]); }
        else throw Error{"unknown projector tensor: " + name};
    }
    else if (starts_with(name, "vision.")) {
        LMX_REQUIRE(cfg.v_layers > 0, "vision tensor given but no vision tower configured: " + name);
        const std::string sub = name.substr(strlen("vision."));
        const int ps = cfg.v_patch_size;
        if (sub == "embeddings.class_embedding") { expect({Dv}); plain(v_cls); }
        else if (sub == "embeddings.patch_embedding.weight") {
            expect({Dv, 3, ps, ps});
            if (!v_patch_w) v_patch_w = alloc_weight((size_t)Dv * kpad * es, true);
            copy_block(v_patch_w, kpad, 0, src, 3 * ps * ps, 0, 0, Dv, 3 * ps * ps, es, st);
        }
        else if (sub == "embeddings.position_embedding.weight") { expect({Tv, Dv}); plain(v_pos); }
        else if (sub == "embeddings.position_ids") { return; }
        else if (sub == "pre_layrnorm.weight") { expect({Dv}); plain(v_pre_w); }
        else if (sub == "pre_layrnorm.bias") { expect({Dv}); plain(v_pre_b); }
        else if (starts_with(sub, "post_layernorm.")) { return; }      // only feeds the unused pooled output
        else if (starts_with(sub, "encoder.layers.")) {
            const size_t p0 = strlen("encoder.layers.");
            const size_t dot = sub.find('.', p0);
            LMX_REQUIRE(dot != std::string::npos, "bad vision layer name " + name);
            const int li = atoi(sub.substr(p0, dot - p0).c_str());
            LMX_REQUIRE(li >= 0 && li < cfg.v_layers, "vision layer index out of range: " + name);
            if (li >= v_run) return;                                    // layers past select_layer are never executed
            const std::string leaf = sub.substr(dot + 1);
            VisLayerW& w = vis[li];
            if (!w.wqkv) { w.wqkv = alloc_weight((size_t)3 * Dv * Dv * es); w.bqkv = alloc_weight((size_t)3 * Dv * es); }
            auto qkv_w = [&](int slot) { expect({Dv, Dv}); copy_block(w.wqkv, Dv, slot * Dv, src, Dv, 0, 0, Dv, Dv, es, st); };
            auto qkv_b = [&](int slot) { expect({Dv}); LMX_CHECK_HIP(hipMemcpyAsync(static_cast<char*>(w.bqkv) + (size_t)slot * Dv * es, src, (size_t)Dv * es, hipMemcpyDeviceToDevice, st)); };
            if (leaf == "self_attn.q_proj.weight") qkv_w(0);
            else if (leaf == "self_attn.k_proj.weight") qkv_w(1);
            else if (leaf == "self_attn.v_proj.weight") qkv_w(2);
            else if (leaf == "self_attn.q_proj.bias") qkv_b(0);
            else if (leaf == "self_attn.k_proj.bias") qkv_b(1);
            else if (leaf == "self_attn.v_proj.bias") qkv_b(2);
            else if (leaf == "self_attn.out_proj.weight") { expect({Dv, Dv}); plain(w.wo); }
            else if (leaf == "self_attn.out_proj.bias") { expect({Dv}); plain(w.bo); }
            else if (leaf == "mlp.fc1.weight") { expect({Fv, Dv}); plain(w.fc1); }
            else if (leaf == "mlp.fc1.bias") { expect({Fv}); plain(w.b1); }
            else if (leaf == "mlp.fc2.weight") { expect({Dv, Fv}); plain(w.fc2); }
            else if (leaf == "mlp.fc2.bias") { expect({Dv}); plain(w.b2); }
            else if (leaf == "layer_norm1.weight") { expect({Dv}); plain(w.ln1w); }
            else if (leaf == "layer_norm1.bias") { expect({Dv}); plain(w.ln1b); }
            else if (leaf == "layer_norm2.weight") { expect({Dv}); plain(w.ln2w); }
            else if (leaf == "layer_norm2.bias") { expect({Dv}); plain(w.ln2b); }
            else throw Error{"unknown vision tensor: " + name};
        }
        else throw Error{"unknown vision tensor: " + name};
    }
    else throw Error{"unknown tensor name: " + name};
    loaded.insert(name);
}

void Model::finalize() {
    std::string missing;
    auto need = [&](const std::string& n) { if (!loaded.count(n)) missing += n + " "; };
    need("model.embed_tokens.weight"); need("model.norm.weight"); need("lm_head.weight");
    for (int i = 0; i < L; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".";
        for (const char* s : {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                              "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight", "input_layernorm.weight",
                              "post_attention_layernorm.weight"})
            need(p + s);
    }
    if (cfg.v_layers > 0) {
        for (const char* s : {"embeddings.class_embedding", "embeddings.patch_embedding.weight", "embeddings.position_embedding.weight",
                              "pre_layrnorm.weight", "pre_layrnorm.bias"})
            need(std::string("vision.") + s);
        for (int i = 0; i < v_run; ++i) {
            const std::string p = "vision.encoder.layers." + std::to_string(i) + ".";
            for (const char* s : {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2",
                                  "layer_norm1", "layer_norm2"}) {
                need(p + s + ".weight"); need(p + s + ".bias");
            }
        }
        for (size_t i = 0; i < proj_w.size(); ++i) {
            const std::string p = cfg.projector_type == LMX_PROJ_LINEAR ? "mm_projector." : "mm_projector." + std::to_string(2 * i) + ".";
            need(p + "weight"); need(p + "bias");
        }
    }
    if (!rope) missing += "<rope table: call lmx_set_rope_table> ";
    if (!missing.empty()) throw Error{"missing tensors: " + missing};
    if (opt_rot) ensure_rot_weights(nullptr);
}

// ---- the decoder's linears (engine.h: DecLinear) ------------------------------------------------------------------------
DecLinear Model::dec_linear(DecSite site, const DecLayerW* w) const {
    const int q_n = nh_l * D, kv_n = 2 * nkv_l * D;
    DecLinear d;
    switch (site) {
        case DecSite::QKV: d.W = w->wqkv; d.Wsw = w->sw_qkv; d.N = d.ldc = qkv_n; d.K = H; d.norm = w->ln1; break;
        case DecSite::Q: d.W = w->wqkv; d.Wrot = w->rot_q; d.N = d.ldc = q_n; d.K = H; d.norm = w->ln1; break;
        case DecSite::KV:      // rows [q_n, q_n + kv_n) of the fused q|k|v weight
            d.W = w->wqkv ? static_cast<const char*>(w->wqkv) + (size_t)q_n * H * es : nullptr; d.Wrot = w->rot_kv; d.N = d.ldc = kv_n; d.K = H; d.norm = w->ln1; break;
        case DecSite::O: d.W = w->wo; d.Wsw = w->sw_o; d.Wrot = w->rot_o; d.N = d.ldc = H; d.K = q_n; d.residual = true; break;
        case DecSite::GateUp: d.W = w->wgu; d.Wsw = w->sw_gu; d.N = 2 * I_l; d.ldc = I_l; d.K = H; d.act = kActSiluMul; d.norm = w->ln2; break;
        case DecSite::Down: d.W = w->wd; d.Wsw = w->sw_d; d.Wrot = w->rot_d; d.N = d.ldc = H; d.K = I_l; d.residual = true; break;
        // vocabulary-parallel head: this rank's V_l rows fill columns [v_off, v_off + V_l) of a [V] row
        case DecSite::Head: d.W = lm_head; d.Wsw = sw_lm_head; d.Wrot = rot_lm_head; d.N = V_l; d.ldc = V; d.c_off = v_off; d.K = H; d.norm = final_norm; break;
    }
    return d;
}

GemvArgs Model::gemv_args(const DecLinear& d, const void* x, void* out) const {
    void* c = out ? static_cast<char*>(out) + (size_t)d.c_off * es : nullptr;
    GemvArgs g{x, d.W, c, nullptr, d.residual && cfg.tp_rank == 0 ? c : nullptr, d.norm, d.norm ? cfg.rms_eps : 0.f, d.N, d.K, d.K, d.K, d.ldc, d.residual ? d.ldc : 0, d.act};
    if (opt_rot && d.Wrot) { g.W = d.Wrot; g.ldw = gemv_rot_pitch(d.K); g.rot = kRotStep; }
    return g;
}

GemmArgs Model::gemm_args(const DecLinear& d, const void* x, void* out, int M) const {
    void* c = static_cast<char*>(out) + (size_t)d.c_off * es;
    return GemmArgs{x, d.W, c, nullptr, d.residual && cfg.tp_rank == 0 ? c : nullptr, M, d.N, d.K, d.K, d.K, d.ldc, d.residual ? d.ldc : 0, d.act};
}

// ---- rotated decode copies (engine.h) ---------------------------------------------------------------------------------
// Each copy is laid out for the rows-per-wave of the launch that reads it: the k|v rows go through the split-q launch (kernels.h), every other site through
// launch_gemv, whose rule reads the very GemvArgs decode_step_launch builds for the site.
int Model::rot_rows(DecSite site, const DecLinear& d) const {
    return site == DecSite::KV ? kDecodeKvRowsPerWave : gemv2_rows_per_wave(gemv_args(d, nullptr, nullptr));
}
void Model::pack_rot(void*& dst, DecSite site, const DecLayerW* w, hipStream_t st) {
    const DecLinear d = dec_linear(site, w);
    if (!d.W) return;
    if (!dst) dst = alloc_weight((size_t)d.N * gemv_rot_pitch(d.K) * es);
    launch_gemv_rot_pack(cfg.dtype, d.W, d.K, dst, d.N, d.K, rot_rows(site, d), kRotStep, false, st);
}

void Model::pack_rot_layer(DecLayerW& w, int which, hipStream_t st) {
    which &= rot_live;
    if (which & kRotDown) pack_rot(w.rot_d, DecSite::Down, &w, st);
    if (which & kRotO) pack_rot(w.rot_o, DecSite::O, &w, st);
    if (which & kRotQ) pack_rot(w.rot_q, DecSite::Q, &w, st);
    if (which & kRotKv) pack_rot(w.rot_kv, DecSite::KV, &w, st);
}
void Model::pack_rot_head(hipStream_t st) {
    if (rot_live & kRotHead) pack_rot(rot_lm_head, DecSite::Head, nullptr, st);
}

void Model::ensure_rot_weights(hipStream_t st) {
    std::lock_guard<std::mutex> lk(mu);
    if (cfg.dtype == kF32) return;
    LMX_CHECK_HIP(hipDeviceSynchronize());                   // the sources may have been written on any stream
    // a copy only where the launch that would read it exists: the hand-counted stream over the packed pitch (32-bit row offsets); q and k|v: the split-q step
    const DecLayerW any;                                     // a site's shape is every layer's
    auto on_copy = [&](DecSite site) { GemvArgs g = gemv_args(dec_linear(site, &any), nullptr, nullptr); g.ldw = gemv_rot_pitch(g.K); return g; };
    auto fits = [&](DecSite site) { return gemv2_applies(cfg.dtype, on_copy(site)); };
    const bool splitq_ok = decode_kv_attn_applies(cfg.dtype, D, on_copy(DecSite::KV)) && s_max % 128 == 0 && s_max / 128 <= 32;
    const int live = (fits(DecSite::Down) ? kRotDown : 0) | (fits(DecSite::O) ? kRotO : 0) | (fits(DecSite::Head) ? kRotHead : 0) | (splitq_ok ? kRotKv : 0) |
                     (splitq_ok && fits(DecSite::Q) ? kRotQ : 0);
    const int fresh = rot_set & live & ~rot_live;            // nothing to do on a second call
    rot_live |= fresh;
    if (!fresh) return;
    for (auto& w : dec) pack_rot_layer(w, fresh, st);
    if (fresh & kRotHead) pack_rot_head(st);
    LMX_CHECK_HIP(hipStreamSynchronize(st));
}

void Model::set_rope(const float* host, int n_pos) {
    LMX_REQUIRE(host != nullptr && n_pos >= s_max, "rope table must cover max_position (rounded up to 64)");
    if (rope) { (void)hipFree(rope); rope = nullptr; }
    LMX_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&rope), (size_t)n_pos * D * sizeof(float)));
    LMX_CHECK_HIP(hipMemcpy(rope, host, (size_t)n_pos * D * sizeof(float), hipMemcpyHostToDevice));
    rope_npos = n_pos;
}

void Model::ensure_comm_stream() {
    std::lock_guard<std::mutex> lk(mu);
    if (!comm_stream) LMX_CHECK_HIP(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
}

void Seq::ensure_events() {
    if (ev_c[0]) return;
    for (int i = 0; i < 2; ++i) {
        LMX_CHECK_HIP(hipEventCreateWithFlags(&ev_c[i], hipEventDisableTiming));
        LMX_CHECK_HIP(hipEventCreateWithFlags(&ev_r[i], hipEventDisableTiming));
    }
}

// ---- one-shot P2P all-reduce plumbing ----------------------------------------------------------------------------------
void Model::p2p_local_handle(void* out64) {
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
    if (!p2p_local) {
        // one allocation: the one-shot region (decode-sized rows) and, behind it, the two-shot region for messages of up to max(s_max, 4096) rows
        p2p_big_max_count = (size_t)std::max(s_max, 4096) * H;
        p2p_big = p2p_big_geometry(cfg.tp_world, p2p_big_max_count, es, p2p_buffer_bytes(cfg.tp_world, H, es));
        const size_t bytes = p2p_big.end;
        // uncached: peers' stores and this rank's flag polls must not sit in a cache while a kernel runs (fine-grained coherent memory where the
        // uncached kind is not available; measured equal, profiles/r04_p2p_mem_ab.txt)
        if (hipExtMallocWithFlags(&p2p_local, bytes, hipDeviceMallocUncached) != hipSuccess) {
            (void)hipGetLastError();
            LMX_CHECK_HIP(hipExtMallocWithFlags(&p2p_local, bytes, hipDeviceMallocFinegrained));
        }
        LMX_CHECK_HIP(hipMemset(p2p_local, 0, bytes));
        LMX_CHECK_HIP(hipDeviceSynchronize());
    }
    hipIpcMemHandle_t hd;
    LMX_CHECK_HIP(hipIpcGetMemHandle(&hd, p2p_local));
    memcpy(out64, &hd, sizeof(hd));
}

void Model::p2p_connect(const void* handles) {
    LMX_REQUIRE(p2p_local != nullptr, "lmx_tp_p2p_connect before lmx_tp_p2p_local_handle");
    LMX_REQUIRE(cfg.tp_world <= P2P_MAX_WORLD, "p2p all-reduce supports up to 8 ranks");
    for (int r = 0; r < cfg.tp_world; ++r) {
        if (r == cfg.tp_rank) { p2p_peer[r] = p2p_local; continue; }
        hipIpcMemHandle_t hd;
        memcpy(&hd, static_cast<const char*>(handles) + (size_t)r * 64, sizeof(hd));
        LMX_CHECK_HIP(hipIpcOpenMemHandle(&p2p_peer[r], hd, hipIpcMemLazyEnablePeerAccess));
    }
    { const char* e = getenv("LMX_TP_P2P_ALL"); p2p_all = e && atoi(e) != 0; }
    { const char* e = getenv("LMX_TP_P2P_BIG"); p2p_big_on = !(e && atoi(e) == 0); }       // 0: prefill-sized messages stay on RCCL (or, with LMX_TP_P2P_ALL, on 32-row one-shot launches)
    p2p_seq = 0; p2p_big_seq = 0;
    p2p_on = true;
}

// 0 = every wait so far saw its flags; otherwise the sequence number of an all-reduce whose wait timed out
int Model::p2p_status(hipStream_t st) {
    if (!p2p_local) return 0;
    uint32_t v = 0;
    const size_t off = p2p_flags_offset(cfg.tp_world, H, es) + (size_t)2 * cfg.tp_world * P2P_MAX_ROWS * 4;
    LMX_CHECK_HIP(hipMemcpyAsync(&v, static_cast<char*>(p2p_local) + off, 4, hipMemcpyDeviceToHost, st));
    LMX_CHECK_HIP(hipStreamSynchronize(st));
    if (v != 0) {
        // report a timeout once, then re-arm: the caller turns it into an error for THIS request; the word would otherwise fail
        // every later generate() on the model although the peers have recovered
        LMX_CHECK_HIP(hipMemsetAsync(static_cast<char*>(p2p_local) + off, 0, 4, st));
        LMX_CHECK_HIP(hipStreamSynchronize(st));
    }
    return (int)v;
}

void Model::allreduce(void* buf, size_t count, hipStream_t st) {
    if (cfg.tp_world == 1 && !comm) return;      // a 1-rank communicator (tests) still goes through RCCL
    if (ar_hook) { ar_hook(buf, (uint64_t)count, cfg.dtype, st, ar_ctx); return; }
    if ((count + H - 1) / H > (size_t)P2P_MAX_ROWS && p2p_big_usable(count)) {
        // prefill-sized message: reduce-scatter + all-gather over all xGMI links in one launch (p2p.hip)
        P2PBigLaunch l{buf, count, cfg.tp_world, cfg.tp_rank, ++p2p_big_seq, p2p_flags_offset(cfg.tp_world, H, es) + (size_t)2 * cfg.tp_world * P2P_MAX_ROWS * 4, {}, p2p_big};
        for (int p = 0; p < cfg.tp_world; ++p) l.peer[p] = p2p_peer[p];
        launch_p2p_allreduce_big(cfg.dtype, l, st);
        return;
    }
    if (p2p_on && count % 8 == 0 && (p2p_all || (count + H - 1) / H <= (size_t)P2P_MAX_ROWS)) {
        // decode-sized message: one launch, one xGMI hop (p2p.hip).  Larger ones only when forced (LMX_TP_P2P_ALL, tests).
        // The message is cut into [H]-element rows (one workgroup each); the last row may be partial (logits: V is not a multiple of H).
        const size_t rows = (count + H - 1) / H;
        for (size_t r0 = 0; r0 < rows; r0 += P2P_MAX_ROWS) {
            const int n = (int)(rows - r0 < (size_t)P2P_MAX_ROWS ? rows - r0 : P2P_MAX_ROWS);
            P2PLaunch l{static_cast<char*>(buf) + r0 * H * es, H, cfg.tp_world, cfg.tp_rank, n, ++p2p_seq, {}};
            for (int p = 0; p < cfg.tp_world; ++p) l.peer[p] = p2p_peer[p];
            if (r0 + n == rows) l.last_len = (int)(count - (rows - 1) * H);
            launch_p2p_allreduce(cfg.dtype, l, st);
        }
        return;
    }
    LMX_REQUIRE(comm != nullptr, "tensor-parallel model used before lmx_tp_init");
    const ncclDataType_t dt = cfg.dtype == kF32 ? ncclFloat32 : cfg.dtype == kBF16 ? ncclBfloat16 : ncclFloat16;
    LMX_CHECK_NCCL(ncclAllReduce(buf, buf, count, dt, ncclSum, comm, st));
}

bool Model::allreduce_norm(void* buf, int rows, const void* norm_w, void* x_out, hipStream_t st) {
    const bool tp = cfg.tp_world > 1 || comm;
    if (tp && !ar_hook && p2p_on && norm_w && x_out && rows >= 1 && rows <= P2P_MAX_ROWS && H % 8 == 0 &&
        !(rows > P2P_MAX_ROWS && p2p_big_usable((size_t)rows * H))) {
        P2PLaunch l{buf, H, cfg.tp_world, cfg.tp_rank, rows, ++p2p_seq, {}};
        for (int p = 0; p < cfg.tp_world; ++p) l.peer[p] = p2p_peer[p];
        l.norm_w = norm_w; l.x_out = x_out; l.eps = cfg.rms_eps;
        launch_p2p_allreduce(cfg.dtype, l, st);
        return true;
    }
    allreduce(buf, (size_t)rows * H, st);
    return false;
}

void Model::gather_logits(void* logits, int rows, hipStream_t st) {
    if (V_l == V) return;
    allreduce(logits, (size_t)rows * V, st);
}

// ---------------------------------------------------------------------------------------------------------------
// vision tower + projector
// ---------------------------------------------------------------------------------------------------------------
void Model::encode_images(const void* pixels, int n, void* feats, hipStream_t st, bool tower_only) {
    LMX_REQUIRE(cfg.v_layers > 0, "no vision tower configured");
    LMX_REQUIRE(n > 0 && pixels && feats, "encode_images: bad arguments");
    std::lock_guard<std::mutex> lk(mu);     // one shared vision workspace
    if (vws_stream && vws_stream != st) LMX_CHECK_HIP(hipStreamWaitEvent(st, vws_done, 0));   // previous user on another stream
    const int dt = cfg.dtype;
    const int rows = n * Tv;                // token rows incl. CLS
    const int prow = n * P;
    const int srows = n * out_tokens;
    const int vh = cfg.v_heads;
    Carve carve;
    const size_t o_patch = carve((size_t)prow * kpad * es), o_pe = carve((size_t)prow * Dv * es), o_h = carve((size_t)rows * Dv * es),
                 o_x = carve((size_t)rows * Dv * es), o_qkv = carve((size_t)rows * 3 * Dv * es), o_attn = carve((size_t)rows * Dv * es),
                 o_mlp = carve((size_t)rows * Fv * es), o_sel = carve((size_t)srows * Dv * es), o_p1 = carve((size_t)srows * H * es),
                 o_p2 = carve((size_t)srows * H * es), o_aws = carve(dt == kF32 ? decode_attn_ws_floats(Tv, vh, 1, vD) * 4 : 0);
    if (carve.off > vws.bytes) { LMX_CHECK_HIP(hipStreamSynchronize(st)); vws.ensure(carve.off); }
    const size_t kv_bytes = (size_t)vh * spad * vD * es;
    if (vkc.bytes < kv_bytes * n) {
        LMX_CHECK_HIP(hipStreamSynchronize(st));
        vkc.ensure(kv_bytes * n, true); vvt.ensure(kv_bytes * n, true);
    }
    char* W = vws.as<char>();
    void *patch = W + o_patch, *pe = W + o_pe, *h = W + o_h, *x = W + o_x, *qkv = W + o_qkv, *attn = W + o_attn, *mlp = W + o_mlp,
         *sel = W + o_sel, *p1 = W + o_p1, *p2 = W + o_p2;
    const int gv = cfg.gemm_variant;

    { LMX_PROF("vis.im2col"); launch_im2col(dt, pixels, patch, n, cfg.v_image_size, cfg.v_patch_size, kpad, st); }
    { LMX_PROF("vis.gemm.patch"); launch_gemm(dt, GemmArgs{patch, v_patch_w, pe, nullptr, nullptr, prow, Dv, kpad, kpad, kpad, Dv, 0, kActNone}, gv, st); }
    { LMX_PROF("vis.embed_ln"); launch_clip_embed_ln(dt, pe, v_cls, v_pos, v_pre_w, v_pre_b, h, n, P, Dv, cfg.v_ln_eps, st); }
    const float scale = 1.f / sqrtf((float)vD);
    for (int l = 0; l < v_run; ++l) {
        const VisLayerW& w = vis[l];
        { LMX_PROF("vis.layernorm"); launch_layernorm(dt, h, w.ln1w, w.ln1b, x, rows, Dv, Dv, Dv, cfg.v_ln_eps, st); }
        // K rows / V^T columns leave the q|k|v GEMM's epilogue (16-bit models; option vis_pack = 0 keeps the separate pack launch: 23 launches of ~5 us per image)
        const bool pack_fused = dt != kF32 && opt_vis_pack && vD % 4 == 0;
        {
            LMX_PROF("vis.gemm.qkv");
            GemmArgs g{x, w.wqkv, qkv, w.bqkv, nullptr, rows, 3 * Dv, Dv, Dv, Dv, 3 * Dv, 0, kActNone};
            if (pack_fused) { g.pk_kc = vkc.p; g.pk_vt = vvt.p; g.pk_heads = vh; g.pk_D = vD; g.pk_rows = Tv; g.pk_spad = spad; g.pk_img_stride = kv_bytes / es; }
            launch_gemm(dt, g, gv, st);
        }
        for (int i = 0; i < n; ++i) {
            char* qkv_i = static_cast<char*>(qkv) + (size_t)i * Tv * 3 * Dv * es;
            char* attn_i = static_cast<char*>(attn) + (size_t)i * Tv * Dv * es;
            void* kc = vkc.as<char>() + (size_t)i * kv_bytes;
            void* vt = vvt.as<char>() + (size_t)i * kv_bytes;
            RopeKvArgs ra{qkv_i, kc, vt, nullptr, nullptr, 0, Tv, 3 * Dv, vh, vh, spad};
            if (!pack_fused) { LMX_PROF("vis.kv_pack"); launch_rope_kv(dt, vD, ra, st); }
            if (dt == kF32) {
                DecodeAttnArgs da{qkv_i, attn_i, kc, vt, nullptr, 0, Tv, Tv, 0, 3 * Dv, Dv, vh, vh, spad, 1, scale,
                                  reinterpret_cast<float*>(W + o_aws)};
                { LMX_PROF("vis.attn"); launch_decode_attn(dt, vD, da, st); }
            } else {
                FlashArgs fa{qkv_i, attn_i, kc, vt, Tv, Tv, 0, 3 * Dv, Dv, vh, vh, spad, scale, 0};
                { LMX_PROF("vis.attn"); launch_flash_prefill(dt, vD, fa, st); }
            }
        }
        { LMX_PROF("vis.gemm.out"); launch_gemm(dt, GemmArgs{attn, w.wo, h, w.bo, h, rows, Dv, Dv, Dv, Dv, Dv, Dv, kActNone}, gv, st); }
        { LMX_PROF("vis.layernorm"); launch_layernorm(dt, h, w.ln2w, w.ln2b, x, rows, Dv, Dv, Dv, cfg.v_ln_eps, st); }
        { LMX_PROF("vis.gemm.fc1"); launch_gemm(dt, GemmArgs{x, w.fc1, mlp, w.b1, nullptr, rows, Fv, Dv, Dv, Dv, Fv, 0, kActQuickGelu}, gv, st); }
        { LMX_PROF("vis.gemm.fc2"); launch_gemm(dt, GemmArgs{mlp, w.fc2, h, w.b2, h, rows, Dv, Fv, Fv, Fv, Dv, Dv, kActNone}, gv, st); }
    }
    // feature_select (clip_encoder.py:29-37)
    const void* selp = h;
    if (cfg.select_feature == LMX_FEATURE_PATCH) { launch_copy_rows(dt, h, sel, n, Tv, 1, P, Dv, st); selp = sel; }
    // projector (multimodal_projector/builder.py:33-51); tower_only: CLIPVisionTower.forward's own result (clip_encoder.py:39-51)
    if (proj_w.empty() || tower_only) {
        LMX_CHECK_HIP(hipMemcpyAsync(feats, selp, (size_t)srows * Dv * es, hipMemcpyDeviceToDevice, st));
    } else {
        const void* in = selp; int in_dim = Dv;
        const int nl = (int)proj_w.size();
        for (int i = 0; i < nl; ++i) {
            void* out = i == nl - 1 ? feats : (i % 2 == 0 ? p1 : p2);
            const int act = i == nl - 1 ? kActNone : kActGeluErf;
            { LMX_PROF("proj.gemm"); launch_gemm(dt, GemmArgs{in, proj_w[i], out, proj_b[i], nullptr, srows, H, in_dim, in_dim, in_dim, H, 0, act}, gv, st); }
            in = out; in_dim = H;
        }
    }
    LMX_CHECK_HIP(hipEventRecord(vws_done, st));
    vws_stream = st;
}

void Model::gather_embeds(const int32_t* src, int rows, const void* feats, void* out, hipStream_t st) {
    LMX_REQUIRE(embed != nullptr, "embed_tokens not loaded");
    launch_gather_embed(cfg.dtype, src, embed, feats, out, rows, H, st);
}

// ---------------------------------------------------------------------------------------------------------------
// sequences
// ---------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_seq_uid{1};

uint64_t next_seq_uid() { return g_seq_uid.fetch_add(1); }

Seq::Seq(Model* mm) : m(mm) {
    uid = g_seq_uid.fetch_add(1);
    layer_stride = (size_t)m->nkv_l * m->s_max * m->D * m->es;
    kc.ensure(layer_stride * m->L, true);
    vt.ensure(layer_stride * m->L, true);
    log_cap = m->s_max + 8;
    state.ensure(16 + (size_t)log_cap * 8, true);
    d_len = state.as<int>(); d_nout = d_len + 1;
    d_tok = reinterpret_cast<int64_t*>(state.as<char>() + 8);
    d_log = d_tok + 1;
    stopbuf.ensure(sizeof(StopSpec), true);
    d_stop = stopbuf.as<StopSpec>();
    // decode workspace
    const int es = m->es;
    n_split = (m->s_max + 127) / 128;          // fixed 128-key chunks (attention.hip: DF_CHUNK)
    const size_t aws = decode_fused_ws_floats(m->nh_l, n_split, m->D);
    Carve carve;
    const size_t o_h = carve((size_t)m->H * es), o_qkv = carve((size_t)m->qkv_n * es), o_attn = carve((size_t)m->nh_l * m->D * es),
                 o_act = carve((size_t)m->I_l * es), o_log = carve((size_t)m->V * es), o_aws = carve(aws * 4), o_cnt = carve((size_t)m->nh_l * 4);
    dws.ensure(carve.off, true);
    char* W = dws.as<char>();
    d_h = W + o_h; d_qkv = W + o_qkv; d_attn = W + o_attn; d_act = W + o_act; d_logits = W + o_log;
    d_aws = reinterpret_cast<float*>(W + o_aws);
    d_cnt = reinterpret_cast<int*>(W + o_cnt);
    kv_gran.ensure((size_t)2 * m->nkv_l * m->D * 8, true);
    LMX_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_status), sizeof(unsigned), hipHostMallocMapped));
    *h_status = 0;
    LMX_CHECK_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_status), h_status, 0));
}

// The rule values travel as a kernel argument; the prompt ids are copied into pinned memory here and from there to the device on `st`, so the caller's
// buffer is free on return and nothing waits for the stream (only a second setter call on the same sequence waits for the first one's copy).
void Seq::set_logit_rules(const LogitRules& r, const int64_t* prompt_host, hipStream_t st) {
    if (logit_rules_neutral(r)) { clear_logit_rules(); return; }
    LMX_REQUIRE(r.n_prompt >= 0 && r.n_prompt <= log_cap, "set_logit_rules: more prompt ids than the sequence's token log holds (max_position + 8)");
    LMX_REQUIRE(r.n_prompt == 0 || prompt_host, "set_logit_rules: null prompt ids");
    LMX_REQUIRE(m->Vr <= RULES_MAX_V, "set_logit_rules: the vocabulary is too large for the logits-processor bitmaps (196608 ids)");
    // First use allocates; each resource is tested on its own, so a call that failed half way leaves nothing the next call would use unallocated.
    // No zero fill: the kernels read promptbuf[0, n_prompt) only, and rulesbuf only after launch_set_logit_rules below has written it.
    if (ev_prompt) { LMX_CHECK_HIP(hipEventSynchronize(ev_prompt)); }          // the previous call's copy has left the staging buffer
    else { LMX_CHECK_HIP(hipEventCreateWithFlags(&ev_prompt, hipEventDisableTiming)); }
    if (!h_prompt) { LMX_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_prompt), (size_t)log_cap * sizeof(int64_t), hipHostMallocDefault)); }
    rulesbuf.ensure(sizeof(LogitRules));
    promptbuf.ensure((size_t)log_cap * sizeof(int64_t));
    if (r.n_prompt > 0) {
        std::memcpy(h_prompt, prompt_host, (size_t)r.n_prompt * sizeof(int64_t));
        LMX_CHECK_HIP(hipMemcpyAsync(promptbuf.p, h_prompt, (size_t)r.n_prompt * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    LMX_CHECK_HIP(hipEventRecord(ev_prompt, st));
    rules = r;
    rules.prompt = promptbuf.as<int64_t>();
    launch_set_logit_rules(rulesbuf.as<LogitRules>(), rules, st);
    rules_on = true;
    last_stream = st; used = true;
    uid = next_seq_uid();          // a decode batch holding this sequence rebuilds its table entry
}

// Attach (cap entries; want_rows: the full fp32 rows too) or, with cap = 0, detach the score log.  Growing a buffer frees the old one, so the stream is drained
// first; the state words are cleared on `st`, ordered with the sequence's work there.
void Seq::set_score_log(int cap, bool want_rows, hipStream_t st) {
    if (cap <= 0) { clear_score_log(); return; }
    LMX_REQUIRE(cap <= log_cap, "set_score_log: more entries than the sequence's token log holds (max_position + 8)");
    const size_t state_off = ((size_t)cap * sizeof(float) + 15) / 16 * 16;
    const size_t need = state_off + 16 + (size_t)m->Vr, need_rows = want_rows ? (size_t)cap * m->Vr * sizeof(float) : 0;
    if (need > scorebuf.bytes || need_rows > score_rows.bytes) {
        LMX_CHECK_HIP(hipStreamSynchronize(st));
        scorebuf.ensure(need);
        if (need_rows) score_rows.ensure(need_rows);
    }
    score_cap = cap; score_rows_on = want_rows;
    LMX_CHECK_HIP(hipMemsetAsync(scorebuf.p, 0, state_off + 16, st));      // logprob = 0, n_scored = 0
    last_stream = st; used = true;
    uid = next_seq_uid();          // a decode batch holding this sequence rebuilds its table entry
}

Seq::~Seq() {
    if (h_prompt) (void)hipHostFree(h_prompt);
    if (ev_prompt) (void)hipEventDestroy(ev_prompt);
    if (h_status) (void)hipHostFree(h_status);
    if (ev_idle) (void)hipEventDestroy(ev_idle);
    for (int i = 0; i < 2; ++i) { if (ev_c[i]) (void)hipEventDestroy(ev_c[i]); if (ev_r[i]) (void)hipEventDestroy(ev_r[i]); }
}

// ---------------------------------------------------------------------------------------------------------------
// prefill
// ---------------------------------------------------------------------------------------------------------------
Model::PrefillWs Model::prefill_ws(Seq* owner, int rows, hipStream_t st) {
    const int dt = cfg.dtype;
    Carve carve;
    const size_t o_h = carve((size_t)rows * H * es), o_x = carve((size_t)rows * H * es), o_qkv = carve((size_t)rows * qkv_n * es),
                 o_attn = carve((size_t)rows * nh_l * D * es), o_act = carve((size_t)rows * I_l * es),
                 o_aws = carve(dt == kF32 ? decode_attn_ws_floats(rows, nh_l, 1, D) * 4 : 0), o_log = carve((size_t)V * es);
    if (carve.off > owner->pws.bytes) { LMX_CHECK_HIP(hipStreamSynchronize(st)); owner->pws.ensure(carve.off); }
    // N = hidden linears (o_proj, down_proj) give too few 256x256 tiles at prompt lengths around 1k: the ping-pong GEMM slices K
    // over up to three workgroups per tile and reduces fp32 partial tiles in the launch (gemm8p.hip).  The scratch is per sequence
    // (request threads prefill concurrently); <= 256 partial tiles = 64 MiB by construction of gemm8p_pick_split.
    if (dt != kF32 && !owner->skw.p) {
        LMX_CHECK_HIP(hipStreamSynchronize(st));
        owner->skw.ensure((size_t)256 * 256 * 256 * sizeof(float));
    }
    char* W = owner->pws.as<char>();
    return PrefillWs{W + o_h, W + o_x, W + o_qkv, W + o_attn, W + o_act, W + o_log, reinterpret_cast<float*>(W + o_aws), owner->skw.p};
}

// Every linear of a piece is a single GEMM over the piece's rows (a 512-row chunk of one request reaches ~0.19 of the MFMA peak, 4096 packed rows
// ~0.4); RoPE / KV append / causal attention run per segment against that segment's own cache.
void Model::prefill_piece(const PrefillWs& ws, const std::vector<PrefillSeg>& seg, int rows, const PieceOpts& o, hipStream_t st) {
    const int dt = cfg.dtype;
    const float scale = 1.f / sqrtf((float)D);
    const int gv = cfg.gemm_variant;
    auto with_scratch = [&](GemmArgs g) { g.skw = ws.skw; return g; };
    auto at = [&](void* base, int r0, size_t width) { return static_cast<char*>(base) + (size_t)r0 * width * es; };
    for (const PrefillSeg& g : seg) LMX_CHECK_HIP(hipMemcpyAsync(at(ws.h, g.row0, H), g.src, (size_t)g.n * H * es, hipMemcpyDeviceToDevice, st));
    // rows [r0, r0+n) of the piece through the attention block / the MLP block of layer l (partial sums land in h)
    auto attn_block = [&](int l, int r0, int n) {
        const DecLayerW& w = dec[l];
        auto kc = [&](const Seq* s) { return s->kc.as<char>() + (size_t)l * s->layer_stride; };
        auto vt = [&](const Seq* s) { return s->vt.as<char>() + (size_t)l * s->layer_stride; };
        void *hr = at(ws.h, r0, H), *xr = at(ws.x, r0, H), *qr = at(ws.qkv, r0, qkv_n), *ar = at(ws.attn, r0, (size_t)nh_l * D);
        { LMX_PROF("prefill.rmsnorm"); launch_rmsnorm(dt, hr, w.ln1, xr, n, H, H, H, cfg.rms_eps, st); }
        // RoPE + KV-cache append ride in the q|k|v GEMM's epilogue where that launch is the un-split ping-pong kernel over head-aligned tiles
        const PrefillSeg& g0 = seg[0];
        const int qpos = g0.pos0 + r0 - g0.row0;
        const bool qf = o.fuse_rope && seg.size() == 1 && gv == 0 && opt_fuse_rope && gemm_fuses_qkv(dt, n, H, D, nh_l, nkv_l, qpos, s_max, false);
        {
            LMX_PROF_K("prefill.gemm.qkv");
            GemmArgs g = with_scratch(gemm_args(dec_linear(DecSite::QKV, &w), xr, qr, n));
            if (qf) { g.qf_rope = rope; g.qf_kc = kc(g0.s); g.qf_vt = vt(g0.s); g.qf_pos0 = qpos; g.qf_nh = nh_l; g.qf_nkv = nkv_l; g.qf_smax = s_max; g.qf_D = D; }
            launch_gemm(dt, g, gv, st);
        }
        for (const PrefillSeg& g : seg) {       // the segment's rows in [r0, r0 + n): rows [a, a + m) of the piece, first position pos
            const int a = std::max(r0, g.row0), m = std::min(r0 + n, g.row0 + g.n) - a, pos = g.pos0 + a - g.row0;
            if (m <= 0) continue;
            void *qa = at(ws.qkv, a, qkv_n), *aa = at(ws.attn, a, (size_t)nh_l * D), *kca = kc(g.s), *vta = vt(g.s);
            if (!qf) { LMX_PROF("prefill.rope_kv"); launch_rope_kv(dt, D, RopeKvArgs{qa, kca, vta, rope, nullptr, pos, m, qkv_n, nh_l, nkv_l, s_max}, st); }
            if (o.attn_probs) {
                void* pl = static_cast<char*>(o.attn_probs) + (size_t)l * nh_l * o.probs_T * o.kv_after * es;
                launch_attn_probs(dt, D, AttnProbsArgs{qa, kca, pl, m, o.probs_c0 + a, o.probs_T, pos, o.kv_after, qkv_n, nh_l, nkv_l, s_max, scale}, st);
            }
            LMX_PROF("prefill.attn");
            if (dt == kF32) launch_decode_attn(dt, D, DecodeAttnArgs{qa, aa, kca, vta, nullptr, pos, m, 0, 1, qkv_n, nh_l * D, nh_l, nkv_l, s_max, 1, scale, ws.aws}, st);
            else launch_flash_prefill(dt, D, FlashArgs{qa, aa, kca, vta, m, pos + m, pos, qkv_n, nh_l * D, nh_l, nkv_l, s_max, scale, 1}, st);
        }
        { LMX_PROF_K("prefill.gemm.o"); launch_gemm(dt, with_scratch(gemm_args(dec_linear(DecSite::O, &w), ar, hr, n)), gv, st); }
    };
    auto mlp_block = [&](int l, int r0, int n) {
        const DecLayerW& w = dec[l];
        void *hr = at(ws.h, r0, H), *xr = at(ws.x, r0, H), *cr = at(ws.act, r0, I_l);
        { LMX_PROF("prefill.rmsnorm"); launch_rmsnorm(dt, hr, w.ln2, xr, n, H, H, H, cfg.rms_eps, st); }
        { LMX_PROF_K("prefill.gemm.gate_up"); launch_gemm(dt, with_scratch(gemm_args(dec_linear(DecSite::GateUp, &w), xr, cr, n)), gv, st); }
        { LMX_PROF_K("prefill.gemm.down"); launch_gemm(dt, with_scratch(gemm_args(dec_linear(DecSite::Down, &w), cr, hr, n)), gv, st); }
    };
    // The two-half pipeline hides 35-55 % of the all-reduce time but costs GEMM efficiency (each half alone cannot fill the chip): measured with a
    // timed stand-in all-reduce (tools/mb_tp_overlap.py, 7B shards) it wins from rows x ranks >= 4096 on — TP=2 at 2048 rows, TP=8 at 1087 —
    // and loses below (TP=2 at 1087 rows: 17.7 vs 15.0 ms serialised).  LMX_TP_OVERLAP=2 forces it (tests), =0 switches it off.
    // With the two-shot peer-to-peer all-reduce (p2p.hip: ~25 us per 8.9 MB message instead of ~114 us on a ring) the sums are 1.6 ms of a TP = 8 prefill:
    // splitting the piece to hide them costs more GEMM efficiency than it can win, so the pipeline is only for the RCCL path (or forced).
    const bool tp_active = cfg.tp_world > 1 || comm != nullptr;
    const bool big_p2p = p2p_big_usable((size_t)rows * H) && rows > P2P_MAX_ROWS && !ar_hook;
    if (o.tp_pipeline && tp_active && tp_overlap && rows >= 256 && !o.hidden && !o.attn_probs &&
        (tp_overlap_force || (!big_p2p && (long)rows * std::max(cfg.tp_world, 1) >= 4096))) {
        // Tensor parallel: the piece runs as two row halves so that the all-reduce of one half (comm stream) overlaps the
        // GEMMs / attention of the other (launch stream).  Half 1's causal attention sees half 0's keys: same-stream order.
        Seq* s = seg[0].s;                  // its events order the two streams
        ensure_comm_stream();
        s->ensure_events();
        const int half0 = round_up((rows + 1) / 2, 128) < rows ? round_up((rows + 1) / 2, 128) : rows / 2;
        const int r0[2] = {0, half0}, rn[2] = {half0, rows - half0};
        auto reduce_async = [&](int i) {
            LMX_CHECK_HIP(hipEventRecord(s->ev_c[i], st));
            LMX_CHECK_HIP(hipStreamWaitEvent(comm_stream, s->ev_c[i], 0));
            { ProfScope ps(this, "prefill.allreduce", comm_stream); allreduce(at(ws.h, r0[i], H), (size_t)rn[i] * H, comm_stream); }
            LMX_CHECK_HIP(hipEventRecord(s->ev_r[i], comm_stream));
        };
        for (int l = 0; l < L; ++l) {
            for (int i = 0; i < 2; ++i) {
                if (l > 0) LMX_CHECK_HIP(hipStreamWaitEvent(st, s->ev_r[i], 0));      // previous layer's MLP sum of this half
                attn_block(l, r0[i], rn[i]);
                reduce_async(i);
            }
            for (int i = 0; i < 2; ++i) {
                LMX_CHECK_HIP(hipStreamWaitEvent(st, s->ev_r[i], 0));
                mlp_block(l, r0[i], rn[i]);
                reduce_async(i);
            }
        }
        for (int i = 0; i < 2; ++i) LMX_CHECK_HIP(hipStreamWaitEvent(st, s->ev_r[i], 0));
        return;
    }
    // output_hidden_states: the piece's rows of entry e of the tuple
    auto hidden_rows = [&](int e) { return static_cast<char*>(o.hidden) + (size_t)e * o.hidden_T * H * es; };
    for (int l = 0; l < L; ++l) {
        if (o.hidden) LMX_CHECK_HIP(hipMemcpyAsync(hidden_rows(l), ws.h, (size_t)rows * H * es, hipMemcpyDeviceToDevice, st));      // the layer's input rows
        attn_block(l, 0, rows);
        allreduce(ws.h, (size_t)rows * H, st);
        mlp_block(l, 0, rows);
        { LMX_PROF_AR("prefill.allreduce"); allreduce(ws.h, (size_t)rows * H, st); }
    }
    if (o.hidden) launch_rmsnorm(dt, ws.h, final_norm, hidden_rows(L), rows, H, H, H, cfg.rms_eps, st);       // the tuple's last entry is normalised
}

void Model::prefill_head(Seq* s, const void* h_row, void* dst, bool pick, hipStream_t st) {
    const int dt = cfg.dtype;
    // vocabulary-parallel head: this rank computes columns [v_off, v_off + V_l) of a zeroed row, the sum over ranks completes it
    if (V_l != V) LMX_CHECK_HIP(hipMemsetAsync(dst, 0, (size_t)V * es, st));
    { LMX_PROF_K("prefill.gemv.lm_head"); launch_gemv(dt, gemv_args(dec_linear(DecSite::Head), h_row, dst), 1, st); }
    gather_logits(dst, 1, st);
    if (!pick) return;
    // with logits processors: the ruled pick (history = the prompt ids + whatever the log holds: nothing, for a request's first token)
    if (s->rules_on) launch_pick_rules(dt, dst, Vr, s->rules, s->d_log, s->log_cap, s->d_nout, 0, s->samp, nullptr, s->d_tok, nullptr, nullptr, st);
    else if (s->samp.temperature > 0.f) launch_sample(dt, dst, Vr, s->samp, s->d_nout, s->d_tok, nullptr, nullptr, st);
    else launch_argmax(dt, dst, Vr, s->d_tok, st);
    launch_log_token(s->d_tok, s->d_log, s->d_nout, s->log_cap, s->d_stop, st);
    record_scores(s, dst, st);
}

// the score recorder behind a pick of one sequence (sampling.hip); nothing is launched for a sequence without a score log
void Model::record_scores(Seq* s, const void* logits, hipStream_t st) {
    if (s->score_cap <= 0) return;
    LMX_PROF("decode.score");
    const SeqStateRef r = s->state_ref();
    const ScoreRef sc = s->score_ref();
    launch_score_record(cfg.dtype, logits, Vr, V, nullptr, &r, nullptr, &sc, 1, s->rules_on, st);
}

// One sequence in pieces of `chunk` rows: each piece is one segment, which may fuse RoPE into the q|k|v GEMM and take the two-half pipeline
void Model::prefill(Seq* s, const void* embeds, int T, int chunk, void* logits, bool logits_all, bool greedy, hipStream_t st, void* hidden, void* attn_probs) {
    LMX_REQUIRE(T > 0 && embeds, "prefill: empty input");
    LMX_REQUIRE(!attn_probs || (cfg.tp_world == 1 && comm == nullptr), "output_attentions: single process only (a tensor-parallel rank holds a slice of the heads)");
    LMX_REQUIRE(s->len + T <= s_max, "prefill: sequence would exceed the KV-cache capacity (max_position)");
    LMX_REQUIRE(rope != nullptr, "rope table not set");
    s->last_stream = st; s->used = true;
    if (chunk <= 0 || chunk > T) chunk = T;
    const int dt = cfg.dtype;
    const PrefillWs ws = prefill_ws(s, chunk, st);
    PieceOpts o;
    o.fuse_rope = o.tp_pipeline = true;
    o.hidden_T = o.probs_T = T;
    o.attn_probs = attn_probs; o.kv_after = s->len + T;      // key range of the attention maps' rows: [0, len + T)
    for (int c0 = 0; c0 < T; c0 += chunk) {
        const int tc = (T - c0) < chunk ? (T - c0) : chunk;
        o.hidden = hidden ? static_cast<char*>(hidden) + (size_t)c0 * H * es : nullptr;
        o.probs_c0 = c0;
        prefill_piece(ws, {PrefillSeg{s, 0, tc, s->len + c0, static_cast<const char*>(embeds) + (size_t)c0 * H * es}}, tc, o, st);
        if (logits_all && logits) {
            char* lc = static_cast<char*>(logits) + (size_t)c0 * V * es;
            launch_rmsnorm(dt, ws.h, final_norm, ws.x, tc, H, H, H, cfg.rms_eps, st);
            if (V_l != V) LMX_CHECK_HIP(hipMemsetAsync(lc, 0, (size_t)tc * V * es, st));
            launch_gemm(dt, gemm_args(dec_linear(DecSite::Head), ws.x, lc, tc), cfg.gemm_variant, st);
            gather_logits(lc, tc, st);
        }
        if (c0 + tc == T && (greedy || (logits && !logits_all)))
            prefill_head(s, static_cast<char*>(ws.h) + (size_t)(tc - 1) * H * es, (logits && !logits_all) ? logits : ws.last_logits, greedy, st);
    }
    s->len += T;
    launch_set_state(s->d_len, s->len, s->d_tok, 0, 0, s->d_nout, -1, st);
}

// ---------------------------------------------------------------------------------------------------------------
// packed prefill of several sequences (serving: BASELINE configs 3 / 4 prefill many requests at once)
// ---------------------------------------------------------------------------------------------------------------
// The rows of all sequences are walked as ONE packed row block in pieces of `block_rows`, one segment per (sequence, row range) in a piece, as in the
// chunked prefill of one sequence.  The row arithmetic is unchanged, so a sequence's result does not depend on who shares the piece with it (up to the
// split-K choice of the N = hidden GEMMs, which changes the summation order of their fp32 partial sums).  Each sequence's last row goes through the
// lm_head and its pick, exactly as Model::prefill does.
void Model::prefill_multi(Seq* const* seqs, const void* const* embeds, const int* Ts, int n, int block_rows, bool greedy, hipStream_t st) {
    LMX_REQUIRE(n >= 1 && seqs && embeds && Ts, "prefill_multi: bad arguments");
    LMX_REQUIRE(rope != nullptr, "rope table not set");
    long total = 0;
    for (int i = 0; i < n; ++i) {
        LMX_REQUIRE(seqs[i] && seqs[i]->m == this && embeds[i] && Ts[i] > 0, "prefill_multi: bad sequence / input");
        LMX_REQUIRE(seqs[i]->len + Ts[i] <= s_max, "prefill_multi: a sequence would exceed the KV-cache capacity (max_position)");
        for (int j = 0; j < i; ++j) LMX_REQUIRE(seqs[j] != seqs[i], "prefill_multi: the same sequence appears twice");
        seqs[i]->last_stream = st; seqs[i]->used = true;
        total += Ts[i];
    }
    if (block_rows <= 0 || block_rows > total) block_rows = (int)total;
    const PrefillWs ws = prefill_ws(seqs[0], block_rows, st);      // the first sequence owns the piece workspace and the split-K scratch of this call
    int cur = 0, cur_done = 0;                                       // next sequence / rows of it already consumed
    while (cur < n) {
        std::vector<PrefillSeg> seg;
        std::vector<int> ends;                                       // segments whose sequence ends in this piece
        int fill = 0;
        while (cur < n && fill < block_rows) {
            const int take = std::min(block_rows - fill, Ts[cur] - cur_done);
            seg.push_back(PrefillSeg{seqs[cur], fill, take, seqs[cur]->len + cur_done, static_cast<const char*>(embeds[cur]) + (size_t)cur_done * H * es});
            fill += take; cur_done += take;
            if (cur_done == Ts[cur]) { ends.push_back((int)seg.size() - 1); ++cur; cur_done = 0; }
        }
        prefill_piece(ws, seg, fill, PieceOpts{}, st);      // no fused RoPE, no two-half pipeline
        if (greedy)
            for (int e : ends) prefill_head(seg[e].s, static_cast<char*>(ws.h) + (size_t)(seg[e].row0 + seg[e].n - 1) * H * es, ws.last_logits, true, st);
    }
    for (int i = 0; i < n; ++i) {
        seqs[i]->len += Ts[i];
        launch_set_state(seqs[i]->d_len, seqs[i]->len, seqs[i]->d_tok, 0, 0, seqs[i]->d_nout, -1, st);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------------------------------
// A bounded in-launch wait of THIS sequence's decode attention timed out (contention from other streams / processes, preemption, a profiler): the step that
// raised the word appended a zero k / v row and merged incomplete partials, so the sequence's output from there on is not valid — the caller's request fails,
// nobody else's.  Reported once: the word and the arrival tickets (which the kernel leaves alone after a timeout) are cleared, and the model stops taking the
// split-q form, whose waiters depend on co-residency with their own launch's projection.
void Seq::check_wait_status(hipStream_t st) {
    if (!h_status || __atomic_load_n(h_status, __ATOMIC_RELAXED) == 0) return;
    __atomic_store_n(h_status, 0u, __ATOMIC_RELAXED);
    m->opt_splitq = false;
    (void)hipMemsetAsync(d_cnt, 0, (size_t)m->nh_l * sizeof(int), st);
    throw Error{"decode step: a bounded in-launch wait of this sequence's attention timed out (decode_attn.hip); its output from that step on is not valid. "
                "The model now uses the separate attention launch (decode_splitq = 0); other sequences are unaffected"};
}

// One decode step of one sequence = per layer {q|k|v projection (+RMSNorm), RoPE + KV append + attention, o_proj (+residual), gate|up (+RMSNorm, SiLU*mul),
// down (+residual)} + lm_head (+final norm) + the pick, as plain stream launches (HF5:models/llama/modeling_llama.py:367-418 for one new token through
// llava_arch.py:103-112).  16-bit models take the split-q form (decode_attn.hip): q alone, then ONE launch holding the attention workgroups and the k|v
// projection, so that the attention's latency chain runs under the k|v weight stream — bit-identical to the three-launch form.
void Model::decode_step_launch(Seq* s, hipStream_t st, int64_t* id_out) {
    const int dt = cfg.dtype;
    const float scale = 1.f / sqrtf((float)D);
    // s->d_h holds the embedding of the token to feed: put there by decode() / decode_batch() before the first step and by the
    // fused pick kernel at the end of every step
    const bool attn16 = (dt == kBF16 || dt == kF16) && s_max % 128 == 0 && s_max / 128 <= 32;      // the chunked launch with the position by value
    for (int l = 0; l < L; ++l) {
        const DecLayerW& w = dec[l];
        void* kc = s->kc.as<char>() + (size_t)l * s->layer_stride;
        void* vt = s->vt.as<char>() + (size_t)l * s->layer_stride;
        DecAttnArgs a{};
        a.qkv = s->d_qkv; a.attn = s->d_attn; a.kc = kc; a.vt = vt; a.rope = rope; a.aws = s->d_aws; a.cnt = s->d_cnt;
        // only the 128-key chunks that exist are launched: the host mirrors the position (s->len == *d_len while this step is queued)
        a.pos = s->len; a.n_split = s->len / 128 + 1; a.nh = nh_l; a.nkv = nkv_l; a.s_max = s_max; a.scale = scale;
        a.status = s->d_status;                      // both forms: the merger's wait for the other chunks is bounded in either
        const GemvArgs gkv = gemv_args(dec_linear(DecSite::KV, &w), s->d_h, nullptr);      // the k | v projection of the split-q form: its rows leave as granules
        if (attn16 && splitq_allowed() && decode_kv_attn_applies(dt, D, gkv)) {
            { LMX_PROF_K("decode.gemv.q"); launch_gemv(dt, gemv_args(dec_linear(DecSite::Q, &w), s->d_h, s->d_qkv), 1, st); }
            a.kv_gran = s->kv_gran.as<unsigned long long>(); a.tag = s->attn_tag;
            if (debug_splitq_timeout.load(std::memory_order_relaxed) > 0 && debug_splitq_timeout.fetch_sub(1) > 0) a.pub_tag = a.tag ^ 0x40000000u;
            s->attn_tag = s->attn_tag >= 0xfffffff0u ? 1u : s->attn_tag + 1;
            { LMX_PROF_K("decode.kv_attn"); launch_decode_kv_attn(dt, D, a, gkv, st); }
        } else {
            { LMX_PROF_K("decode.gemv.qkv"); launch_gemv(dt, gemv_args(dec_linear(DecSite::QKV, &w), s->d_h, s->d_qkv), 1, st); }
            LMX_PROF("decode.attn");
            if (attn16) launch_decode_attn_step(dt, D, a, st);
            else {
                DecodeFusedArgs fa{s->d_qkv, kc, vt, rope, s->d_len, nh_l, nkv_l, s_max, s->len / 128 + 1, scale, s->d_aws, s->d_cnt, s->d_attn};
                launch_decode_fused(dt, D, fa, st);
            }
        }
        { LMX_PROF_K("decode.gemv.o"); launch_gemv(dt, gemv_args(dec_linear(DecSite::O, &w), s->d_attn, s->d_h), 1, st); }
        { LMX_PROF_AR("decode.allreduce"); allreduce(s->d_h, (size_t)H, st); }
        { LMX_PROF_K("decode.gemv.gate_up"); launch_gemv(dt, gemv_args(dec_linear(DecSite::GateUp, &w), s->d_h, s->d_act), 1, st); }
        { LMX_PROF_K("decode.gemv.down"); launch_gemv(dt, gemv_args(dec_linear(DecSite::Down, &w), s->d_act, s->d_h), 1, st); }
        allreduce(s->d_h, (size_t)H, st);
    }
    if (V_l != V) LMX_CHECK_HIP(hipMemsetAsync(s->d_logits, 0, (size_t)V * es, st));
    { LMX_PROF_K("decode.gemv.lm_head"); launch_gemv(dt, gemv_args(dec_linear(DecSite::Head), s->d_h, s->d_logits), 1, st); }
    { ProfScope ps_ag(this, V_l != V ? "decode.allgather.logits" : nullptr, st); gather_logits(s->d_logits, 1, st); }
    {
        LMX_PROF("decode.argmax");      // pick (argmax | draw) + *len += 1 + token log + next token's embedding row -> d_h, one launch
        const SeqStateRef r = s->state_ref();
        launch_argmax_advance_batch(dt, s->d_logits, Vr, V, nullptr, &r, 1, id_out, embed, s->d_h, H, st, s->rules_on);      // id_out: the picked id, or -1 once the stop rule has fired
    }
    record_scores(s, s->d_logits, st);      // the next step's lm_head overwrites d_logits only behind it on the stream
}

void Model::seq_copy(Seq* dst, const Seq* src, hipStream_t st) {
    LMX_REQUIRE(dst && src && dst->m == this && src->m == this && dst != src, "seq_copy: bad sequences");
    LMX_REQUIRE(src->len > 0, "seq_copy: the source has no context");
    const size_t n = (size_t)src->len;
    // K rows [L][kv_head][s_max][D]: n * D contiguous elements per (layer, head);  V^T [L][kv_head][D][s_max]: n contiguous elements per (layer, head, d)
    LMX_CHECK_HIP(hipMemcpy2DAsync(dst->kc.p, (size_t)s_max * D * es, src->kc.p, (size_t)s_max * D * es, n * D * es, (size_t)L * nkv_l, hipMemcpyDeviceToDevice, st));
    LMX_CHECK_HIP(hipMemcpy2DAsync(dst->vt.p, (size_t)s_max * es, src->vt.p, (size_t)s_max * es, n * es, (size_t)L * nkv_l * D, hipMemcpyDeviceToDevice, st));
    dst->len = src->len;
    launch_set_state(dst->d_len, dst->len, dst->d_tok, 0, 0, dst->d_nout, 0, st);
    dst->last_stream = st; dst->used = true;
}

void Model::decode(Seq* s, int64_t token, int n_steps, void* logits, bool greedy, hipStream_t st) {
    LMX_REQUIRE(n_steps >= 1, "decode: n_steps must be >= 1");
    LMX_REQUIRE(greedy || n_steps == 1, "decode: chained steps need greedy sampling on the device");
    LMX_REQUIRE(s->len + n_steps <= s_max, "decode: sequence would exceed the KV-cache capacity (max_position)");
    LMX_REQUIRE(s->len > 0, "decode before prefill");
    LMX_REQUIRE(token < V, "token id out of range");
    s->last_stream = st; s->used = true;
    if (token >= 0) launch_set_state(s->d_len, -1, s->d_tok, token, 1, s->d_nout, -1, st);
    // Plain stream launches: the ~160 kernels of a step average >20 us each against ~3.5 us of host launch cost, so the
    // host runs far ahead of the GPU; a captured hipGraph measured no faster (3.57 vs 3.56 ms/token, profiles/EXPERIMENTS.md)
    // and stream capture is not safe next to other threads using the legacy stream (model_worker runs 5 request threads).
    { LMX_PROF("decode.embed"); launch_gather_token(cfg.dtype, s->d_tok, embed, s->d_h, H, V, st); }
    for (int i = 0; i < n_steps; ++i) {
        decode_step_launch(s, st);
        s->len += 1;
    }
    if (logits) LMX_CHECK_HIP(hipMemcpyAsync(logits, s->d_logits, (size_t)V * es, hipMemcpyDeviceToDevice, st));
}

// ---------------------------------------------------------------------------------------------------------------
// decode batch (continuous batching): several sequences, each with its own KV cache and position, advance
// one token per step and share ONE pass over the weights.
// ---------------------------------------------------------------------------------------------------------------
// Decode-batch weights: the skinny MFMA kernel loads its A fragments per lane, so from the [N][K] layout every 16-lane group of a load
// touches 16 different rows (uncoalesced: 3.3-4.4 TB/s).  With 288 GB of HBM the decoder weights are simply kept a second time in
// fragment order (13 GB at 7B), where each load instruction of a wave reads 1 KiB of contiguous memory.  LMX_BATCH_SWIZZLE=0 disables.
void Model::ensure_batch_weights(hipStream_t st) {
    std::lock_guard<std::mutex> lk(mu);
    if (batch_weights_ready) return;
    batch_weights_ready = true;
    const char* e = getenv("LMX_BATCH_SWIZZLE");
    if (cfg.dtype == kF32 || (e && atoi(e) == 0)) return;
    auto mk = [&](const DecLinear& d) -> void* {
        if (!d.W) return nullptr;
        void* sw = alloc_weight(skinny_swizzled_bytes(d.N, d.K, es));
        launch_skinny_swizzle(cfg.dtype, d.W, d.K, sw, d.N, d.K, st);
        return sw;
    };
    for (auto& w : dec) {
        w.sw_qkv = mk(dec_linear(DecSite::QKV, &w));
        w.sw_o = mk(dec_linear(DecSite::O, &w));
        w.sw_gu = mk(dec_linear(DecSite::GateUp, &w));
        w.sw_d = mk(dec_linear(DecSite::Down, &w));
    }
    sw_lm_head = mk(dec_linear(DecSite::Head));
    LMX_CHECK_HIP(hipStreamSynchronize(st));
}

Batch::Batch(Model* mm, int capacity) : m(mm), cap(capacity) {
    LMX_REQUIRE(capacity >= 1 && capacity <= 256, "batch capacity must be 1..256");
    const int es = m->es;
    Carve carve;
    const size_t o_h = carve((size_t)cap * m->H * es), o_x = carve((size_t)cap * m->H * es), o_qkv = carve((size_t)cap * m->qkv_n * es),
                 o_attn = carve((size_t)cap * m->nh_l * m->D * es), o_act = carve((size_t)cap * m->I_l * es), o_log = carve((size_t)cap * m->V * es);
    ws.ensure(carve.off, true);
    char* W = ws.as<char>();
    h = W + o_h; x = W + o_x; qkv = W + o_qkv; attn = W + o_attn; act = W + o_act; logits = W + o_log;
    const size_t attn_bytes = sizeof(DecodeFusedSeq) * (size_t)m->L * cap, state_bytes = sizeof(SeqStateRef) * (size_t)cap;
    tab.ensure(attn_bytes + state_bytes, true);
    score_tab.ensure(sizeof(ScoreRef) * (size_t)cap, true);
    host_score_tab.resize((size_t)cap);
    if (m->cfg.dtype != kF32) {                     // K-sliced linears of a decode batch: o_proj / down_proj (N = H) and q|k|v
        const int nmax = std::max(m->H, m->qkv_n);
        sk_scratch.ensure(skinny_scratch_bytes(nmax)); sk_cnt.ensure((size_t)(nmax / 64 + 1) * sizeof(int), true);
    }
    d_attn_tab = tab.as<DecodeFusedSeq>();
    d_state_tab = reinterpret_cast<SeqStateRef*>(tab.as<char>() + attn_bytes);
    host_tab.resize(attn_bytes + state_bytes);
}

// (re)build the device tables when the membership changed since the last step
void Batch::bind(Seq* const* seqs, int n, hipStream_t st) {
    bool same = (int)members.size() == n;
    for (int i = 0; same && i < n; ++i) same = members[(size_t)i] == seqs[i]->uid;
    if (same) return;
    const int L = m->L;
    DecodeFusedSeq* at = reinterpret_cast<DecodeFusedSeq*>(host_tab.data());
    SeqStateRef* stt = reinterpret_cast<SeqStateRef*>(host_tab.data() + sizeof(DecodeFusedSeq) * (size_t)L * cap);
    for (int i = 0; i < n; ++i) {
        Seq* s = seqs[i];
        for (int l = 0; l < L; ++l)
            at[(size_t)l * cap + i] = DecodeFusedSeq{s->kc.as<char>() + (size_t)l * s->layer_stride, s->vt.as<char>() + (size_t)l * s->layer_stride,
                                                     s->d_len, s->d_aws, s->d_cnt};
        stt[i] = s->state_ref();
        host_score_tab[(size_t)i] = s->score_ref();
    }
    // the previous step's kernels may still be reading the old tables on this stream, and the host image is reused
    LMX_CHECK_HIP(hipStreamSynchronize(st));
    LMX_CHECK_HIP(hipMemcpyAsync(tab.p, host_tab.data(), host_tab.size(), hipMemcpyHostToDevice, st));
    LMX_CHECK_HIP(hipMemcpyAsync(score_tab.p, host_score_tab.data(), sizeof(ScoreRef) * (size_t)n, hipMemcpyHostToDevice, st));
    LMX_CHECK_HIP(hipStreamSynchronize(st));
    members.resize((size_t)n);
    for (int i = 0; i < n; ++i) members[(size_t)i] = seqs[i]->uid;
}

void Model::decode_batch(Batch* b, Seq* const* seqs, int n, const int64_t* tokens, int n_steps, void* logits, bool greedy, int64_t* ids_out_host, hipStream_t st,
                         bool sync_ids) {
    LMX_REQUIRE(b && b->m == this, "decode_batch: batch belongs to another model");
    LMX_REQUIRE(n >= 1 && n <= b->cap, "decode_batch: number of sequences exceeds the batch capacity");
    LMX_REQUIRE(n_steps >= 1, "decode_batch: n_steps must be >= 1");
    LMX_REQUIRE(greedy || n_steps == 1, "decode_batch: chained steps need greedy sampling on the device");
    for (int i = 0; i < n; ++i) {
        Seq* s = seqs[i];
        LMX_REQUIRE(s && s->m == this, "decode_batch: sequence belongs to another model");
        LMX_REQUIRE(s->len > 0, "decode before prefill");
        LMX_REQUIRE(s->len + n_steps <= s_max, "decode_batch: a sequence would exceed the KV-cache capacity (max_position)");
        for (int j = 0; j < i; ++j) LMX_REQUIRE(seqs[j] != s, "decode_batch: the same sequence appears twice");
        if (tokens) LMX_REQUIRE(tokens[i] < V, "token id out of range");
        s->last_stream = st; s->used = true;
    }
    if (n > 1) ensure_batch_weights(st);
    b->bind(seqs, n, st);
    bool any_rules = false;        // per launch: the rules-carrying pick only when some member has logits processors
    bool any_scores = false;       // per launch: the score recorder only when some member has a score log
    for (int i = 0; i < n; ++i) { any_rules = any_rules || seqs[i]->rules_on; any_scores = any_scores || seqs[i]->score_cap > 0; }
    if (n_steps > b->ids_steps) { LMX_CHECK_HIP(hipStreamSynchronize(st)); b->ids.ensure((size_t)n_steps * b->cap * 8); b->ids_steps = n_steps; }
    int64_t* d_ids = b->ids.as<int64_t>();
    if (tokens)
        for (int i = 0; i < n; ++i)
            if (tokens[i] >= 0) launch_set_state(seqs[i]->d_len, -1, seqs[i]->d_tok, tokens[i], 1, seqs[i]->d_nout, -1, st);

    const int dt = cfg.dtype;
    const float scale = 1.f / sqrtf((float)D);
    // A batch row-block linear y = act(norm(x) W^T) (+ residual): rmsnorm launch + the skinny MFMA kernel on the fragment-order weight
    // copy for up to 32 rows (7B, per step: 2 rows ~3.3 ms, 8 rows 4.2 ms, 32 rows 8.8 ms; the multi-row GEMV chain measured 3.75 ms at
    // 2 rows and 5.05 ms at 4, so it is not used); fp32 verification engine / larger batches: prefill GEMM family.
    // x_ready: b->x already holds the normalised rows (allreduce_norm's hand-over); otherwise a linear with a norm in front takes b->h through it into b->x
    auto linear = [&](const DecLinear& d, const void* x, bool x_ready, void* out) {
        if (d.norm && !x_ready) {
            LMX_PROF("decode_batch.rmsnorm");
            launch_rmsnorm(dt, x, d.norm, b->x, n, d.K, d.K, d.K, cfg.rms_eps, st);
            x = b->x;
        }
        LMX_PROF("decode_batch.linear");
        GemmArgs g = gemm_args(d, x, out, n);
        if (dt != kF32 && g.M <= 32) { g.Wsw = d.Wsw; g.skw = b->sk_scratch.p; g.sk_cnt = b->sk_cnt.as<int>(); launch_skinny_gemm(dt, g, st); } else launch_gemm(dt, g, cfg.gemm_variant, st);
    };
    if (n == 1) {
        // a lone member takes the single-sequence step (GEMV with fused RMSNorm: fewer launches, full-rate weight stream)
        Seq* s = seqs[0];
        launch_gather_token(dt, s->d_tok, embed, s->d_h, H, V, st);
        for (int step = 0; step < n_steps; ++step) {
            decode_step_launch(s, st, d_ids + (size_t)step * b->cap);      // a lone member reports -1 after a device-side stop exactly like the members of a larger batch
            s->len += 1;
        }
        if (logits) LMX_CHECK_HIP(hipMemcpyAsync(logits, s->d_logits, (size_t)V * es, hipMemcpyDeviceToDevice, st));
    } else {
    { LMX_PROF("decode_batch.embed"); launch_gather_tokens_batch(dt, b->d_state_tab, n, embed, b->h, H, V, st); }
    for (int step = 0; step < n_steps; ++step) {
        bool x_ready = false;          // b->x already holds the normalised rows of the NEXT linear (written by the tensor-parallel all-reduce's launch: allreduce_norm)
        for (int l = 0; l < L; ++l) {
            const DecLayerW& w = dec[l];
            linear(dec_linear(DecSite::QKV, &w), x_ready ? b->x : b->h, x_ready, b->qkv);
            {
                LMX_PROF("decode_batch.attn");
                int max_len = 0;
                for (int i = 0; i < n; ++i) max_len = std::max(max_len, seqs[i]->len);
                // live 128-key chunks of the longest member (the host mirrors every position); shorter members' surplus workgroups only take their ticket
                DecodeFusedArgs a{b->qkv, nullptr, nullptr, rope, nullptr, nh_l, nkv_l, s_max, max_len / 128 + 1, scale, nullptr, nullptr, b->attn};
                a.tab = b->d_attn_tab + (size_t)l * b->cap; a.n_seq = n; a.qkv_stride = qkv_n; a.o_stride = nh_l * D;
                launch_decode_fused(dt, D, a, st);
            }
            linear(dec_linear(DecSite::O, &w), b->attn, false, b->h);
            { LMX_PROF_AR("decode_batch.allreduce"); x_ready = allreduce_norm(b->h, n, w.ln2, b->x, st); }
            linear(dec_linear(DecSite::GateUp, &w), x_ready ? b->x : b->h, x_ready, b->act);
            linear(dec_linear(DecSite::Down, &w), b->act, false, b->h);
            x_ready = allreduce_norm(b->h, n, l + 1 < L ? dec[l + 1].ln1 : final_norm, b->x, st);       // the next layer's input norm (or the final one) rides in the same launch
        }
        if (V_l != V) LMX_CHECK_HIP(hipMemsetAsync(b->logits, 0, (size_t)n * V * es, st));
        linear(dec_linear(DecSite::Head), x_ready ? b->x : b->h, x_ready, b->logits);
        gather_logits(b->logits, n, st);
        // pick + advance + the picked tokens' embedding rows -> b->h (input of the next step), one launch
        { LMX_PROF("decode_batch.argmax"); launch_argmax_advance_batch(dt, b->logits, Vr, V, b->d_state_tab, nullptr, n, d_ids + (size_t)step * b->cap, embed, b->h, H, st, any_rules); }
        if (any_scores) { LMX_PROF("decode_batch.score"); launch_score_record(dt, b->logits, Vr, V, b->d_state_tab, nullptr, b->score_tab.as<ScoreRef>(), nullptr, n, any_rules, st); }
        for (int i = 0; i < n; ++i) seqs[i]->len += 1;
    }
    }
    if (logits && n > 1) LMX_CHECK_HIP(hipMemcpyAsync(logits, b->logits, (size_t)n * V * es, hipMemcpyDeviceToDevice, st));
    if (ids_out_host) {       // [n_steps][n], after the stream drained
        LMX_CHECK_HIP(hipMemcpy2DAsync(ids_out_host, (size_t)n * 8, d_ids, (size_t)b->cap * 8, (size_t)n * 8, (size_t)n_steps, hipMemcpyDeviceToHost, st));
        if (sync_ids) {
            LMX_CHECK_HIP(hipStreamSynchronize(st));
            // a member whose id rule fired reports -1 from then on and its device position stands still: bring the host mirror back to it
            for (int i = 0; i < n; ++i) {
                int live = 0;
                for (int step = 0; step < n_steps; ++step) live += ids_out_host[(size_t)step * n + i] >= 0;
                seqs[i]->len -= n_steps - live;
            }
        }
    }
}

}  // namespace lmx
