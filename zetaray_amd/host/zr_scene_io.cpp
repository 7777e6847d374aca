// zr_scene_io.cpp -- see zr_scene_io.h.  Plain C++17, no HIP, no third-party parser (the reference uses cgltf; the subset of glTF 2.0 it
// consumes -- external buffers, TRS / matrix nodes, indexed triangle primitives, pbrMetallicRoughness + four KHR material extensions -- is
// small enough for the JSON reader below).
#include "zr_scene_io.h"
#include "../../include/zr_detmath.h"
#include "../../include/zr_scene_math.h"
#include "../../include/zr_anim.h"
#include "../../include/zr_skin.h"
#include "../../include/zr_morph.h"
#include "../../include/zr_bcn.h"
#include "../../include/zr_texture.h"
#include "../../include/zr_mipgen.h"
#include "../../include/zr_jpeg.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace {

// Mat43 / FromToWorld / DecomposeSRT / FillMeshInstance / the EmissiveTriangle encode, decode and transform: one statement for the host and the device
using namespace zrsm;
using namespace zran;

thread_local std::string g_err;
struct Error { std::string what; };
[[noreturn]] void Throw(const std::string& s) { throw Error{s}; }

// ------------------------------------------------------------------------------------------------ JSON
struct Json
{
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    bool b = false; double num = 0; std::string str;
    std::vector<Json> arr; std::vector<std::pair<std::string, Json>> obj;
    const Json* Find(const char* k) const { for (auto& kv : obj) if (kv.first == k) return &kv.second; return nullptr; }
    const Json& At(const char* k) const { const Json* j = Find(k); if (!j) Throw(std::string("glTF: missing key '") + k + "'"); return *j; }
    double NumOr(const char* k, double d) const { const Json* j = Find(k); return (j && j->kind == Num) ? j->num : d; }
    int IntOr(const char* k, int d) const { const Json* j = Find(k); return (j && j->kind == Num) ? (int)j->num : d; }
    bool BoolOr(const char* k, bool d) const { const Json* j = Find(k); return (j && j->kind == Bool) ? j->b : d; }
    std::string StrOr(const char* k, const char* d) const { const Json* j = Find(k); return (j && j->kind == Str) ? j->str : std::string(d); }
    size_t Size() const { return kind == Arr ? arr.size() : 0; }
};
struct JsonParser
{
    const char* p; const char* end;
    void Ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) p++; }
    [[noreturn]] void Bad(const char* w) { Throw(std::string("JSON: ") + w); }
    Json Value()
    {
        Ws(); if (p >= end) Bad("unexpected end");
        Json j;
        if (*p == '{')
        {
            j.kind = Json::Obj; p++; Ws();
            if (p < end && *p == '}') { p++; return j; }
            for (;;)
            {
                Ws(); if (p >= end || *p != '"') Bad("expected a key");
                std::string k = String(); Ws();
                if (p >= end || *p != ':') Bad("expected ':'");
                p++;
                j.obj.emplace_back(std::move(k), Value()); Ws();
                if (p < end && *p == ',') { p++; continue; }
                if (p < end && *p == '}') { p++; return j; }
                Bad("expected ',' or '}'");
            }
        }
        if (*p == '[')
        {
            j.kind = Json::Arr; p++; Ws();
            if (p < end && *p == ']') { p++; return j; }
            for (;;)
            {
                j.arr.push_back(Value()); Ws();
                if (p < end && *p == ',') { p++; continue; }
                if (p < end && *p == ']') { p++; return j; }
                Bad("expected ',' or ']'");
            }
        }
        if (*p == '"') { j.kind = Json::Str; j.str = String(); return j; }
        if (!strncmp(p, "true", 4) && end - p >= 4) { j.kind = Json::Bool; j.b = true; p += 4; return j; }
        if (!strncmp(p, "false", 5) && end - p >= 5) { j.kind = Json::Bool; j.b = false; p += 5; return j; }
        if (!strncmp(p, "null", 4) && end - p >= 4) { p += 4; return j; }
        char* e = nullptr; j.num = strtod(p, &e);
        if (e == p) Bad("unexpected character");
        j.kind = Json::Num; p = e; return j;
    }
    std::string String()
    {
        std::string s; p++;
        while (p < end && *p != '"')
        {
            if (*p == '\\' && p + 1 < end)
            {
                p++;
                switch (*p) { case 'n': s += '\n'; break; case 't': s += '\t'; break; case 'r': s += '\r'; break; case 'b': s += '\b'; break; case 'f': s += '\f'; break;
                case 'u': { unsigned c = 0; if (end - p < 5) Bad("bad \\u escape"); sscanf(p + 1, "%4x", &c); p += 4; if (c < 0x80) s += (char)c; else if (c < 0x800) { s += (char)(0xc0 | (c >> 6)); s += (char)(0x80 | (c & 63)); } else { s += (char)(0xe0 | (c >> 12)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); } break; }
                default: s += *p; }
                p++;
            }
            else s += *p++;
        }
        if (p >= end) Bad("unterminated string");
        p++; return s;
    }
};

std::vector<uint8_t> ReadFile(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) Throw("cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
std::string DirOf(const std::string& p) { size_t i = p.find_last_of('/'); return i == std::string::npos ? std::string(".") : p.substr(0, i); }

// ------------------------------------------------------------------------------------------------ packing helpers (Material.h, Vector.h)
uint32_t Unorm8(float f) { f = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f); return (uint32_t)(f * 255.0f + 0.5f); }
uint32_t Rgb8(const float* c) { return Unorm8(c[0]) | (Unorm8(c[1]) << 8) | (Unorm8(c[2]) << 16); }      // Float3ToRGB8
// (EncodeOct32 -- Math::encode_octahedral + unorm2::FromNormalized -- is in zr_scene_math.h)

struct MaterialDesc      // glTF::Asset::MaterialDesc defaults (Material.h:66-95 via pack below)
{
    float baseColor[4] = {1, 1, 1, 1}; float metallic = 1.0f, roughness = 1.0f, ior = 1.5f, transmission = 0.0f, subsurface = 0.0f;
    float coatWeight = 0.0f, coatColor[3] = {0.8f, 0.8f, 0.8f}, coatRoughness = 0.0f, coatIor = 1.6f;
    float emissiveFactor[3] = {0, 0, 0}; float emissiveStrength = 1.0f, normalScale = 1.0f, alphaCutoff = 0.5f; int alphaMode = 0;
    bool doubleSided = false, thinWalled = false; float transmissionDepth = 0.0f;
    uint32_t baseColorTex = 0xffff, normalTex = 0xffff, mrTex = 0xffff, emissiveTex = 0xffff;
};
// the setters of Material (Source/ZetaCore/Core/Material.h:66-260), as zetaray_amd/scene_io.py pack_material states them
zr_material PackMaterial(const MaterialDesc& d)
{
    zr_material m; std::memset(&m, 0, sizeof(m));
    m.base_color_factor = Rgb8(d.baseColor) | (Unorm8(d.baseColor[3]) << 24);
    m.base_color_tex_subsurf_coat_weight = d.baseColorTex | (Unorm8(d.subsurface) << 16) | (Unorm8(d.coatWeight) << 24);
    m.normal_tex_tr_depth = d.normalTex | ((uint32_t)zr_f32_to_f16(d.transmissionDepth) << 16);
    m.mr_tex_spec_roughness_coat_roughness = d.mrTex | (Unorm8(d.roughness) << 16) | (Unorm8(d.coatRoughness) << 24);
    m.emissive_factor_normal_scale = Rgb8(d.emissiveFactor) | (Unorm8(d.normalScale) << 24);
    float iorN = (d.ior - 1.0f) / 1.5f; iorN = iorN < 0.0f ? 0.0f : (iorN > 1.0f ? 1.0f : iorN);
    m.emissive_strength_ior = (uint32_t)zr_f32_to_f16(d.emissiveStrength) | ((uint32_t)(iorN * 65535.0f + 0.5f) << 16);
    m.emissive_tex_alpha_cutoff_coat_ior = d.emissiveTex | (Unorm8(d.alphaCutoff) << 16) | (Unorm8((d.coatIor - 1.0f) / 1.5f) << 24);
    uint32_t flags = Rgb8(d.coatColor);
    if (d.metallic >= 0.9f) flags |= 1u << ZR_MAT_METALLIC_BIT;
    if (d.doubleSided) flags |= 1u << ZR_MAT_DOUBLE_SIDED_BIT;
    if (d.transmission >= 0.9f) flags |= 1u << ZR_MAT_TRANSMISSIVE_BIT;
    flags |= ((uint32_t)d.alphaMode & 3u) << 27;
    if (d.thinWalled) flags |= 1u << ZR_MAT_THIN_WALLED_BIT;
    m.coat_color_flags = flags;
    return m;
}

// ------------------------------------------------------------------------------------------------ transforms (Math/MatrixFuncs.h)
// Mat43 (zr_scene_math.h): row-vector 4 x 4 as the reference stores it, rows 0-2 = images of the basis vectors, row 3 = translation
// ToToWorld, RotationMatFromQuat, AffineTransformation and Mul are include/zr_anim.h's (namespace zran): the device form of the animation compiles them too

// RT::EmissiveTriangle ctor + StoreVertices (RtCommon.h:73-190)
void PackEmissiveTriangle(const float* v0, const float* v1, const float* v2, const float* uv, uint32_t factorRGB8, uint32_t tex, uint16_t strengthH,
    uint32_t id, bool doubleSided, zr_emissive_triangle& e)
{
    std::memset(&e, 0, sizeof(e));
    StoreEmissiveVertices(e, v0, v1, v2);
    e.id = id;
    e.packed_a = (factorRGB8 & 0xffffffu) | (1u << 24) | (doubleSided ? (1u << 25) : 0u) | (((uint32_t)strengthH & 0xfu) << 28);
    e.packed_b = (tex & 0xffffu) | ((uint32_t)strengthH << 16);
    for (int k = 0; k < 2; k++) { e.uv0[k] = zr_f32_to_f16(uv[k]); e.uv1[k] = zr_f32_to_f16(uv[2 + k]); e.uv2[k] = zr_f32_to_f16(uv[4 + k]); }
}

// ------------------------------------------------------------------------------------------------ block decompression
// BC7 (BPTC) and BC5: include/zr_bcn.h, the header the device form of the decode (zr_tu_texdecode.hip) compiles too
using zrbc::Bc7Block; using zrbc::Bc4Block;

// ------------------------------------------------------------------------------------------------ DDS -> texel heap entry
// keep: ZR_TEX_SRC_BC7 / ZR_TEX_SRC_BC5 -- a file of that encoding is NOT decoded: `chain` gets its blocks, every mip back to back as the file stores them,
// and `mip` stays empty (ZRH_LOAD_KEEP_COMPRESSED); ZR_TEX_SRC_RAW decodes everything, as zrh_gltf_load does
struct Image { uint32_t w = 0, h = 0, mips = 0; int channels = 4; bool srgbFormat = false; std::vector<std::vector<uint8_t>> mip; std::vector<uint8_t> chain; };
Image LoadDDS(const std::string& path, int keep = ZR_TEX_SRC_RAW)
{
    const std::vector<uint8_t> d = ReadFile(path);
    if (d.size() < 128 || std::memcmp(d.data(), "DDS ", 4)) Throw(path + ": not a DDS file");
    auto u32 = [&](size_t off) { uint32_t v; std::memcpy(&v, d.data() + off, 4); return v; };
    Image img; img.h = u32(12); img.w = u32(16); img.mips = u32(28) ? u32(28) : 1;
    // zr_texture_desc stores 16-bit dimensions and an 8-bit mip count; a full chain of a 65535-texel side has 16 levels
    if (img.w == 0 || img.h == 0 || img.w > 65535u || img.h > 65535u) Throw(path + ": texture dimensions must be in [1, 65535]");
    if (img.mips > 16u) Throw(path + ": more than 16 mip levels");
    size_t off = 128; uint32_t fmt = 0;
    if (!std::memcmp(d.data() + 84, "DX10", 4)) { fmt = u32(128); off = 148; }
    else if (!std::memcmp(d.data() + 84, "ATI2", 4) || !std::memcmp(d.data() + 84, "BC5U", 4)) fmt = 83;
    else Throw(path + ": only DX10-header or BC5 DDS files are supported");
    // DXGI_FORMAT: 28 / 29 RGBA8 (UNORM / sRGB), 83 BC5_UNORM, 98 / 99 BC7 (UNORM / sRGB)
    if (fmt != 28 && fmt != 29 && fmt != 83 && fmt != 98 && fmt != 99) Throw(path + ": unsupported DXGI format " + std::to_string(fmt));
    img.channels = fmt == 83 ? 2 : 4; img.srgbFormat = (fmt == 29 || fmt == 99);
    uint32_t w = img.w, h = img.h;
    const bool kept = (keep == ZR_TEX_SRC_BC7 && (fmt == 98 || fmt == 99)) || (keep == ZR_TEX_SRC_BC5 && fmt == 83);
    for (uint32_t m = 0; m < img.mips; m++)
    {
        const uint32_t bw = (w + 3) / 4, bh = (h + 3) / 4;
        const size_t bytes = fmt == 28 || fmt == 29 ? (size_t)w * h * 4 : (size_t)bw * bh * 16;
        if (off + bytes > d.size()) Throw(path + ": truncated");
        if (kept) { img.chain.insert(img.chain.end(), d.begin() + off, d.begin() + off + bytes); off += bytes; w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1; continue; }
        std::vector<uint8_t> px((size_t)w * h * img.channels);
        if (fmt == 28 || fmt == 29) std::memcpy(px.data(), d.data() + off, bytes);
        else if (fmt == 83) zrh_bc5_decode(d.data() + off, w, h, px.data());
        else zrh_bc7_decode(d.data() + off, w, h, px.data());
        img.mip.push_back(std::move(px));
        off += bytes; w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1;
    }
    return img;
}

// ------------------------------------------------------------------------------------------------ PNG -> RGBA8
// What a stock glTF carries.  No link dependency: inflate (RFC 1951: stored, fixed and dynamic Huffman blocks), the zlib wrapper with its Adler-32
// (RFC 1950) and the chunk CRC-32 are written here.  Every read is bounds-checked: a corrupted file is refused or decoded within the buffers.
uint32_t Crc32(const uint8_t* p, size_t n)
{
    struct Table { uint32_t t[256]; Table() { for (uint32_t i = 0; i < 256u; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1; t[i] = c; } } };
    static const Table table;
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = table.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c ^ 0xffffffffu;
}
uint32_t Adler32(const uint8_t* p, size_t n)
{
    uint32_t a = 1u, b = 0u;
    while (n)
    {
        const size_t k = n < 5552u ? n : 5552u;      // the longest run whose sums stay below 2^32
        for (size_t i = 0; i < k; i++) { a += p[i]; b += a; }
        a %= 65521u; b %= 65521u; p += k; n -= k;
    }
    return (b << 16) | a;
}
// a zlib stream -> `out`, which must come to exactly `expect` bytes
struct Inflater
{
    const std::string& name; const uint8_t* in; size_t inLen; std::vector<uint8_t>& out; size_t expect;
    size_t inPos = 0; uint32_t bitBuf = 0; int bitCnt = 0;
    struct Huff { uint16_t count[16]; uint16_t symbol[288]; };
    [[noreturn]] void Bad(const char* why) { Throw(name + ": " + why); }
    uint32_t Bits(int need)      // need <= 16; fewer than 8 bits are ever left in bitBuf
    {
        uint32_t v = bitBuf;
        while (bitCnt < need) { if (inPos >= inLen) Bad("truncated: the compressed data ends early"); v |= (uint32_t)in[inPos++] << bitCnt; bitCnt += 8; }
        bitBuf = v >> need; bitCnt -= need;
        return v & ((1u << need) - 1u);
    }
    void Build(Huff& h, const uint8_t* lengths, int n)
    {
        std::memset(&h, 0, sizeof(h));
        for (int i = 0; i < n; i++) h.count[lengths[i]]++;
        int left = 1;
        for (int len = 1; len < 16; len++) { left <<= 1; left -= h.count[len]; if (left < 0) Bad("invalid deflate data: over-subscribed Huffman code"); }
        uint16_t offs[16]; offs[1] = 0;
        for (int len = 1; len < 15; len++) offs[len + 1] = (uint16_t)(offs[len] + h.count[len]);
        for (int i = 0; i < n; i++) if (lengths[i]) h.symbol[offs[lengths[i]]++] = (uint16_t)i;
    }
    int Decode(const Huff& h)
    {
        int code = 0, first = 0, index = 0;
        for (int len = 1; len < 16; len++)
        {
            code |= (int)Bits(1);
            const int count = h.count[len];
            if (code - count < first) return h.symbol[index + (code - first)];
            index += count; first += count; first <<= 1; code <<= 1;
        }
        Bad("invalid deflate data: no such Huffman code");
    }
    void Put(uint8_t b) { if (out.size() >= expect) Bad("the compressed data holds more than the image"); out.push_back(b); }
    void Codes(const Huff& lencode, const Huff& distcode)
    {
        static const uint16_t lens[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        static const uint16_t dists[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        for (;;)
        {
            int sym = Decode(lencode);
            if (sym < 256) { Put((uint8_t)sym); continue; }
            if (sym == 256) return;
            sym -= 257;
            if (sym >= 29) Bad("invalid deflate data: bad length symbol");
            const size_t len = lens[sym] + Bits(lext[sym]);
            const int ds = Decode(distcode);
            if (ds >= 30) Bad("invalid deflate data: bad distance symbol");
            const size_t dist = dists[ds] + Bits(dext[ds]);
            if (dist > out.size()) Bad("invalid deflate data: distance beyond the start");
            if (len > expect - out.size()) Bad("the compressed data holds more than the image");
            for (size_t i = 0; i < len; i++) out.push_back(out[out.size() - dist]);
        }
    }
    void Run()
    {
        if (inLen < 2) Bad("truncated: no zlib header");
        const uint32_t cmf = in[0], flg = in[1];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 32u)) Bad("invalid zlib header");
        inPos = 2;
        for (uint32_t last = 0; !last;)
        {
            last = Bits(1);
            const uint32_t type = Bits(2);
            if (type == 0)
            {
                bitBuf = 0; bitCnt = 0;
                if (inLen - inPos < 4) Bad("truncated: the compressed data ends early");
                const uint32_t len = in[inPos] | (in[inPos + 1] << 8), nlen = in[inPos + 2] | (in[inPos + 3] << 8);
                inPos += 4;
                if ((len ^ 0xffffu) != nlen) Bad("invalid deflate data: stored block length");
                if (len > inLen - inPos) Bad("truncated: the compressed data ends early");
                if (len > expect - out.size()) Bad("the compressed data holds more than the image");
                out.insert(out.end(), in + inPos, in + inPos + len); inPos += len;
            }
            else if (type == 1)
            {
                uint8_t l[288 + 30];
                for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8));
                for (int i = 0; i < 30; i++) l[288 + i] = 5;
                Huff lencode, distcode; Build(lencode, l, 288); Build(distcode, l + 288, 30);
                Codes(lencode, distcode);
            }
            else if (type == 2)
            {
                static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                const int nlen = (int)Bits(5) + 257, ndist = (int)Bits(5) + 1, ncode = (int)Bits(4) + 4;
                if (nlen > 286 || ndist > 30) Bad("invalid deflate data: too many codes");
                uint8_t l[286 + 30]; std::memset(l, 0, sizeof(l));
                for (int i = 0; i < ncode; i++) l[order[i]] = (uint8_t)Bits(3);
                Huff lencode, distcode; Build(lencode, l, 19);
                std::memset(l, 0, sizeof(l));
                for (int i = 0; i < nlen + ndist;)
                {
                    const int sym = Decode(lencode);
                    if (sym < 16) { l[i++] = (uint8_t)sym; continue; }
                    uint8_t v = 0; int rep;
                    if (sym == 16) { if (i == 0) Bad("invalid deflate data: repeat without a length"); v = l[i - 1]; rep = 3 + (int)Bits(2); }
                    else if (sym == 17) rep = 3 + (int)Bits(3);
                    else rep = 11 + (int)Bits(7);
                    if (i + rep > nlen + ndist) Bad("invalid deflate data: too many lengths");
                    while (rep--) l[i++] = v;
                }
                if (!l[256]) Bad("invalid deflate data: no end-of-block code");
                uint8_t dl[30]; std::memcpy(dl, l + nlen, (size_t)ndist);
                Build(lencode, l, nlen); Build(distcode, dl, ndist);
                Codes(lencode, distcode);
            }
            else Bad("invalid deflate data: block type 3");
        }
        if (out.size() != expect) Bad("truncated: the compressed data holds less than the image");
        if (inLen - inPos < 4) Bad("truncated: no Adler-32");
        const uint32_t want = ((uint32_t)in[inPos] << 24) | ((uint32_t)in[inPos + 1] << 16) | ((uint32_t)in[inPos + 2] << 8) | in[inPos + 3];
        if (Adler32(out.data(), out.size()) != want) Bad("bad Adler-32");
    }
};

// bit depth 8 and 16 (the high byte is kept), colour types 0, 2, 3 (with tRNS), 4 and 6, the five row filters; no interlacing
struct Png { uint32_t w = 0, h = 0; std::vector<uint8_t> rgba; };
Png DecodePng(const std::string& name, const uint8_t* d, size_t n)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    if (n < 8 || std::memcmp(d, sig, 8)) Throw(name + ": not a PNG file");
    auto be32 = [&](size_t off) { return ((uint32_t)d[off] << 24) | ((uint32_t)d[off + 1] << 16) | ((uint32_t)d[off + 2] << 8) | (uint32_t)d[off + 3]; };
    Png png; uint32_t depth = 0, ctype = 0; bool haveHdr = false, end = false;
    std::vector<uint8_t> idat, plte, trns;
    for (size_t at = 8; !end;)
    {
        if (n - at < 12) Throw(name + ": truncated: the file ends without IEND");
        const uint32_t len = be32(at);
        if (len > n - at - 12) Throw(name + ": truncated: a chunk is longer than the file");
        const uint8_t* type = d + at + 4; const uint8_t* body = d + at + 8;
        if (Crc32(type, 4u + len) != be32(at + 8 + len)) Throw(name + ": bad CRC in chunk " + std::string((const char*)type, 4));
        const bool is = haveHdr || !std::memcmp(type, "IHDR", 4);
        if (!is) Throw(name + ": the first chunk is not IHDR");
        if (!std::memcmp(type, "IHDR", 4))
        {
            if (haveHdr || len != 13) Throw(name + ": invalid IHDR");
            png.w = be32(at + 8); png.h = be32(at + 12); depth = body[8]; ctype = body[9];
            if (png.w == 0 || png.h == 0 || png.w > 65535u || png.h > 65535u) Throw(name + ": texture dimensions must be in [1, 65535]");
            if (depth == 1 || depth == 2 || depth == 4) Throw(name + ": bit depths below 8 are not supported");
            if ((depth != 8 && depth != 16) || (ctype != 0 && ctype != 2 && ctype != 3 && ctype != 4 && ctype != 6) || (ctype == 3 && depth != 8)) Throw(name + ": invalid bit depth / colour type");
            if (body[10] != 0 || body[11] != 0) Throw(name + ": invalid compression / filter method");
            if (body[12] == 1) Throw(name + ": interlaced PNG files are not supported");
            if (body[12] != 0) Throw(name + ": invalid interlace method");
            haveHdr = true;
        }
        else if (!std::memcmp(type, "PLTE", 4)) { if (len % 3u || len > 768u || len == 0) Throw(name + ": invalid PLTE"); plte.assign(body, body + len); }
        else if (!std::memcmp(type, "tRNS", 4)) trns.assign(body, body + len);
        else if (!std::memcmp(type, "IDAT", 4)) idat.insert(idat.end(), body, body + len);
        else if (!std::memcmp(type, "IEND", 4)) end = true;
        at += 12u + (size_t)len;
    }
    if (!haveHdr || idat.empty()) Throw(name + ": truncated: no image data");
    const uint32_t channels = ctype == 0 ? 1u : (ctype == 2 ? 3u : (ctype == 3 ? 1u : (ctype == 4 ? 2u : 4u))), bps = depth / 8u, bpp = channels * bps;
    const size_t stride = (size_t)png.w * bpp, expect = (size_t)png.h * (stride + 1u);
    // (deflate expands by at most 1032 : 1: a header that promises more than the data can hold is refused before anything is allocated)
    if (expect / 1032u > idat.size()) Throw(name + ": truncated: the compressed data holds less than the image");
    if (ctype == 3 && plte.empty()) Throw(name + ": palette image without PLTE");
    if ((ctype == 0 && !trns.empty() && trns.size() != 2) || (ctype == 2 && !trns.empty() && trns.size() != 6) || (ctype == 3 && trns.size() > plte.size() / 3u)) Throw(name + ": invalid tRNS");
    std::vector<uint8_t> raw;
    Inflater inf{name, idat.data(), idat.size(), raw, expect};
    inf.Run();
    // the row filters, in place
    for (uint32_t y = 0; y < png.h; y++)
    {
        uint8_t* cur = raw.data() + (size_t)y * (stride + 1u) + 1u; const uint8_t* prev = y ? cur - (stride + 1u) : nullptr;
        const uint8_t f = cur[-1];
        if (f > 4) Throw(name + ": invalid row filter");
        for (size_t i = 0; i < stride; i++)
        {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0, c = (prev && i >= bpp) ? prev[i - bpp] : 0;
            int pred = 0;
            if (f == 1) pred = a;
            else if (f == 2) pred = b;
            else if (f == 3) pred = (a + b) >> 1;
            else if (f == 4) { const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c); pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
            cur[i] = (uint8_t)(cur[i] + pred);
        }
    }
    png.rgba.resize((size_t)png.w * png.h * 4u);
    for (uint32_t y = 0; y < png.h; y++)
    {
        const uint8_t* row = raw.data() + (size_t)y * (stride + 1u) + 1u; uint8_t* o = png.rgba.data() + (size_t)y * png.w * 4u;
        for (uint32_t x = 0; x < png.w; x++, o += 4)
        {
            const uint8_t* s = row + (size_t)x * bpp;      // sample k is s[k bps]: the high byte of a 16-bit sample comes first
            if (ctype == 3)
            {
                const uint32_t idx = s[0];
                if (idx >= plte.size() / 3u) Throw(name + ": palette index out of range");
                o[0] = plte[3u * idx]; o[1] = plte[3u * idx + 1u]; o[2] = plte[3u * idx + 2u]; o[3] = idx < trns.size() ? trns[idx] : 255;
            }
            else if (ctype == 0 || ctype == 4)
            {
                o[0] = o[1] = o[2] = s[0];
                if (ctype == 4) o[3] = s[bps];
                else o[3] = (!trns.empty() && (bps == 2 ? (s[0] == trns[0] && s[1] == trns[1]) : s[0] == trns[1])) ? 0 : 255;
            }
            else
            {
                o[0] = s[0]; o[1] = s[bps]; o[2] = s[2u * bps];
                if (ctype == 6) o[3] = s[3u * bps];
                else
                {
                    bool key = !trns.empty();
                    for (uint32_t k = 0; key && k < 3u; k++) key = bps == 2 ? (s[2u * k] == trns[2u * k] && s[2u * k + 1u] == trns[2u * k + 1u]) : s[k] == trns[2u * k + 1u];
                    o[3] = key ? 0 : 255;
                }
            }
        }
    }
    return png;
}
bool EndsWith(const std::string& s, const char* ext)      // ASCII case-insensitive
{
    const size_t n = std::strlen(ext);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; i++) { char c = s[s.size() - n + i]; if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a'); if (c != ext[i]) return false; }
    return true;
}
// a .png image as the one-level Image of its slot: RGBA8 as decoded, or the two channels an RG8 slot keeps (r0, r1 of the file's R, G, B, A)
Image LoadPNG(const std::string& path, bool colour, uint32_t r0, uint32_t r1)
{
    const std::vector<uint8_t> d = ReadFile(path);
    Png png = DecodePng(path, d.data(), d.size());
    Image img; img.w = png.w; img.h = png.h; img.channels = colour ? 4 : 2; img.srgbFormat = colour;
    img.mips = 1; for (uint32_t m = png.w > png.h ? png.w : png.h; m > 1u; m >>= 1) img.mips++;      // 1 + floor(log2(max(w, h)))
    if (colour) img.mip.push_back(std::move(png.rgba));
    else
    {
        std::vector<uint8_t> rg((size_t)png.w * png.h * 2u);
        for (size_t i = 0; i < (size_t)png.w * png.h; i++) { rg[2u * i] = png.rgba[4u * i + r0]; rg[2u * i + 1u] = png.rgba[4u * i + r1]; }
        img.mip.push_back(std::move(rg));
    }
    return img;
}

// ------------------------------------------------------------------------------------------------ JPEG -> the record of include/zr_jpeg.h
// The sequential part of a baseline JPEG: markers, tables and the Huffman-coded scan, into the record the header (here) or the kernels of zr_tu_jpeg.hip
// turn into texels.  SOF0 / SOF1, 8 bits, 1 or 3 components (4:4:4, 4:2:2, 4:2:0), one scan, DRI / RSTn.  Every read is bounds-checked.
struct JpegReader
{
    const std::string& name; const uint8_t* d; size_t n;
    size_t pos = 0; uint32_t buf = 0; int cnt = 0, fake = 0;      // buf: the next cnt bits, left-aligned; the last `fake` of them are zeros fed behind the data's end
    struct Huff { bool set = false; uint8_t count[17] = {}; uint8_t symbol[256] = {}; int32_t maxcode[18] = {}; int32_t valptr[17] = {}; uint16_t fast[512] = {}; };
    Huff dc[4], ac[4];
    [[noreturn]] void Bad(const char* why) { Throw(name + ": " + why); }
    void Build(Huff& h, const uint8_t* counts, const uint8_t* symbols, uint32_t total)
    {
        h = Huff();
        int32_t code = 0; uint32_t p = 0;
        for (int len = 1; len <= 16; len++)
        {
            h.count[len] = counts[len - 1]; h.valptr[len] = (int32_t)p - code;
            if (code + (int32_t)counts[len - 1] > (1 << len)) Bad("invalid DHT: over-subscribed Huffman code");
            for (uint32_t i = 0; i < counts[len - 1]; i++, p++, code++)
            {
                h.symbol[p] = symbols[p];
                if (len <= 9) for (int32_t f = code << (9 - len); f < ((code + 1) << (9 - len)); f++) h.fast[f] = (uint16_t)((len << 8) | symbols[p]);
            }
            h.maxcode[len] = counts[len - 1] ? code - 1 : -1;
            code <<= 1;
        }
        h.maxcode[17] = 0x7fffffff; h.set = true; (void)total;
    }
    void Fill()
    {
        while (cnt <= 24)
        {
            uint32_t b = 0;
            if (pos < n && !(d[pos] == 0xffu && (pos + 1 >= n || d[pos + 1] != 0u))) { b = d[pos]; pos += b == 0xffu ? 2u : 1u; }
            else fake += 8;      // a marker or the end of the file: zeros, counted
            buf |= b << (24 - cnt); cnt += 8;
        }
    }
    void Drop(int bits) { buf <<= bits; cnt -= bits; if (cnt < fake) Bad("truncated: the entropy-coded data ends early"); }
    uint32_t Bits(int need)      // need <= 16
    {
        if (!need) return 0u;
        Fill();
        const uint32_t v = buf >> (32 - need);
        Drop(need);
        return v;
    }
    uint32_t Decode(const Huff& h)
    {
        Fill();
        const uint32_t f = h.fast[buf >> 23];
        if (f) { Drop((int)(f >> 8)); return f & 0xffu; }
        for (int len = 10; len <= 16; len++)
        {
            const int32_t code = (int32_t)(buf >> (32 - len));
            if (code <= h.maxcode[len]) { Drop(len); return h.symbol[(code + h.valptr[len]) & 0xff]; }
        }
        Bad("invalid entropy-coded data: a Huffman code that is not in the table");
    }
    static int32_t Extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int32_t)v - (int32_t)((1u << s) - 1u) : (int32_t)v; }
    // one block into blk[0 .. 63] (zigzag order, zeroed here); returns n = the index of the last non-zero coefficient + 1, at least 1
    uint32_t Block(const Huff& hd, const Huff& ha, uint32_t& pred, int16_t* blk)
    {
        std::memset(blk, 0, 64 * sizeof(int16_t));
        const uint32_t s = Decode(hd);
        if (s > 11u) Bad("invalid entropy-coded data: a DC difference of more than 11 bits");
        pred += (uint32_t)Extend(Bits((int)s), (int)s);
        blk[0] = (int16_t)pred;
        uint32_t last = 0u;
        for (uint32_t k = 1; k < 64u;)
        {
            const uint32_t rs = Decode(ha), r = rs >> 4, sz = rs & 15u;
            if (!sz)
            {
                if (r != 15u) break;      // end of block
                k += 16u;
                if (k > 64u) Bad("invalid entropy-coded data: a coefficient index past 63");
                continue;
            }
            k += r;
            if (k > 63u) Bad("invalid entropy-coded data: a coefficient index past 63");
            blk[k] = (int16_t)Extend(Bits((int)sz), (int)sz);
            last = k++;
        }
        return last + 1u;
    }
};
struct JpegPacked { zrjp::Header hdr; std::vector<uint32_t> begin; std::vector<int16_t> coef; };
JpegPacked PackJpeg(const std::string& name, const uint8_t* d, size_t n, uint32_t map)
{
    JpegReader rd{name, d, n};
    if (n < 4 || d[0] != 0xffu || d[1] != 0xd8u) Throw(name + ": not a JPEG file");
    JpegPacked out; std::memset(&out.hdr, 0, sizeof(out.hdr));
    zrjp::Header& hdr = out.hdr;
    hdr.magic = zrjp::kMagic; hdr.map = map;
    uint16_t qt[4][64]; bool haveQt[4] = {false, false, false, false};
    uint8_t compId[3] = {0, 0, 0}, compTq[3] = {0, 0, 0};
    bool haveFrame = false; int adobe = -1; uint32_t restart = 0;
    size_t at = 2;
    auto be16 = [&](size_t off) { return ((uint32_t)d[off] << 8) | d[off + 1]; };
    for (;;)
    {
        if (at >= n || d[at] != 0xffu) Throw(name + ": truncated or corrupt: no marker where one must stand");
        while (at < n && d[at] == 0xffu) at++;      // (fill bytes)
        if (at >= n) Throw(name + ": truncated: the file ends before the scan");
        const uint32_t m = d[at++];
        if (m == 0xd9u) Throw(name + ": truncated: no scan before the end of the image");
        if (m == 0x01u || (m >= 0xd0u && m <= 0xd7u)) continue;      // (stand-alone markers)
        if (n - at < 2) Throw(name + ": truncated: a marker segment is cut off");
        const uint32_t len = be16(at);
        if (len < 2u || len > n - at) Throw(name + ": truncated: a marker segment is longer than the file");
        const uint8_t* seg = d + at + 2; const uint32_t segLen = len - 2u;
        if (m == 0xc2u) Throw(name + ": progressive JPEG files are not supported");
        if (m == 0xc9u || m == 0xcau || m == 0xcbu || m == 0xccu || m == 0xcdu || m == 0xceu || m == 0xcfu) Throw(name + ": arithmetic-coded JPEG files are not supported");
        if (m == 0xc3u || m == 0xc5u || m == 0xc6u || m == 0xc7u || m == 0xdeu) Throw(name + ": lossless / hierarchical JPEG files are not supported");
        if (m == 0xc0u || m == 0xc1u)
        {
            if (haveFrame) Throw(name + ": more than one frame header");
            if (segLen < 6u) Throw(name + ": invalid frame header");
            if (seg[0] == 12u) Throw(name + ": 12-bit JPEG files are not supported");
            if (seg[0] != 8u) Throw(name + ": invalid sample precision");
            hdr.h = be16(at + 3); hdr.w = be16(at + 5); hdr.ncomp = seg[5];
            if (hdr.w == 0u || hdr.h == 0u) Throw(name + ": texture dimensions must be in [1, 65535]");
            if (hdr.ncomp == 4u) Throw(name + ": 4-component (CMYK / YCCK) JPEG files are not supported");
            if (hdr.ncomp != 1u && hdr.ncomp != 3u) Throw(name + ": invalid component count");
            if (segLen != 6u + 3u * hdr.ncomp) Throw(name + ": invalid frame header");
            for (uint32_t c = 0; c < hdr.ncomp; c++)
            {
                compId[c] = seg[6u + 3u * c]; compTq[c] = seg[8u + 3u * c];
                hdr.comp[c].hs = seg[7u + 3u * c] >> 4; hdr.comp[c].vs = seg[7u + 3u * c] & 15u;
                if (compTq[c] > 3u) Throw(name + ": invalid quantisation table selector");
            }
            if (hdr.ncomp == 1u) hdr.comp[0].hs = hdr.comp[0].vs = 1u;      // (a single component is not interleaved: its sampling factors mean nothing)
            if (!zrjp::LayoutComponents(hdr)) Throw(name + ": unsupported chroma sampling (4:4:4, 4:2:2 and 4:2:0 are read)");
            haveFrame = true;
        }
        else if (m == 0xc4u)
        {
            for (uint32_t p = 0; p < segLen;)
            {
                if (segLen - p < 17u) Throw(name + ": invalid DHT");
                const uint32_t tc = seg[p] >> 4, th = seg[p] & 15u;
                uint32_t total = 0; for (uint32_t i = 0; i < 16u; i++) total += seg[p + 1u + i];
                if (tc > 1u || th > 3u || total > 256u || segLen - p - 17u < total) Throw(name + ": invalid DHT");
                rd.Build(tc ? rd.ac[th] : rd.dc[th], seg + p + 1u, seg + p + 17u, total);
                p += 17u + total;
            }
        }
        else if (m == 0xdbu)
        {
            for (uint32_t p = 0; p < segLen;)
            {
                const uint32_t pq = seg[p] >> 4, tq = seg[p] & 15u;
                if (pq > 1u || tq > 3u || segLen - p - 1u < 64u * (pq + 1u)) Throw(name + ": invalid DQT");
                for (uint32_t k = 0; k < 64u; k++) qt[tq][k] = pq ? (uint16_t)((seg[p + 1u + 2u * k] << 8) | seg[p + 2u + 2u * k]) : seg[p + 1u + k];
                haveQt[tq] = true; p += 1u + 64u * (pq + 1u);
            }
        }
        else if (m == 0xddu) { if (segLen != 2u) Throw(name + ": invalid DRI"); restart = be16(at + 2); }
        else if (m == 0xeeu && segLen >= 12u && !std::memcmp(seg, "Adobe", 5)) adobe = seg[11];
        else if (m == 0xdau)
        {
            if (!haveFrame) Throw(name + ": a scan before the frame header");
            if (segLen < 1u || segLen != 4u + 2u * seg[0]) Throw(name + ": invalid scan header");
            if (seg[0] != hdr.ncomp) Throw(name + ": JPEG files with several scans are not supported");
            if (hdr.ncomp == 3u && adobe == 0) Throw(name + ": RGB (Adobe transform 0) JPEG files are not supported");
            const JpegReader::Huff* hd[3]; const JpegReader::Huff* ha[3];
            for (uint32_t c = 0; c < hdr.ncomp; c++)
            {
                if (seg[1u + 2u * c] != compId[c]) Throw(name + ": the scan names its components in another order than the frame");
                const uint32_t td = seg[2u + 2u * c] >> 4, ta = seg[2u + 2u * c] & 15u;
                if (td > 3u || ta > 3u || !rd.dc[td].set || !rd.ac[ta].set) Throw(name + ": the scan names a Huffman table the file does not define");
                hd[c] = &rd.dc[td]; ha[c] = &rd.ac[ta];
                if (!haveQt[compTq[c]]) Throw(name + ": the frame names a quantisation table the file does not define");
                std::memcpy(hdr.comp[c].q, qt[compTq[c]], sizeof(qt[0]));
            }
            if (seg[segLen - 3u] != 0u || seg[segLen - 2u] != 63u || seg[segLen - 1u] != 0u) Throw(name + ": invalid spectral selection for a sequential scan");
            at += len;
            // (a block is at least a 1-bit DC code and a 1-bit end of block: a header that promises more than the data can hold is refused before
            // anything is allocated)
            if ((uint64_t)hdr.num_blocks > 4ull * (n - at)) Throw(name + ": truncated: the header promises more blocks than the data can hold");
            // the scan: MCU by MCU, each block appended in scan order; `slot` says where it stands in the record
            const uint32_t B = hdr.num_blocks, hs = hdr.comp[0].hs, vs = hdr.comp[0].vs;
            const uint32_t mcusX = hdr.comp[0].bw / hs, mcusY = hdr.comp[0].bh / vs;
            std::vector<uint32_t> scanBegin; scanBegin.reserve((size_t)B + 1u); std::vector<uint32_t> slot; slot.reserve(B);
            std::vector<int16_t> scanCoef; scanCoef.reserve((size_t)B * 4u);
            rd.pos = at;
            uint32_t pred[3] = {0, 0, 0}, sinceRestart = 0, nextRst = 0;
            int16_t blk[64];
            for (uint32_t my = 0; my < mcusY; my++) for (uint32_t mx = 0; mx < mcusX; mx++)
            {
                if (restart && sinceRestart == restart)
                {   // byte-align; what is left of the last byte is padding, and RSTn stands next
                    if (rd.cnt - rd.fake >= 8) Throw(name + ": bad or missing restart marker");
                    size_t p = rd.pos;
                    while (p + 1 < n && d[p] == 0xffu && d[p + 1] == 0xffu) p++;
                    if (p + 1 >= n || d[p] != 0xffu || d[p + 1] != 0xd0u + nextRst) Throw(name + ": bad or missing restart marker");
                    rd.pos = p + 2; rd.buf = 0; rd.cnt = 0; rd.fake = 0;
                    nextRst = (nextRst + 1u) & 7u; sinceRestart = 0; pred[0] = pred[1] = pred[2] = 0;
                }
                sinceRestart++;
                for (uint32_t c = 0; c < hdr.ncomp; c++) for (uint32_t v = 0; v < hdr.comp[c].vs; v++) for (uint32_t h = 0; h < hdr.comp[c].hs; h++)
                {
                    const uint32_t nz = rd.Block(*hd[c], *ha[c], pred[c], blk);
                    if (scanCoef.size() + nz > 0xffffffffull) Throw(name + ": more than 2^32 - 1 coefficients");
                    scanBegin.push_back((uint32_t)scanCoef.size());
                    scanCoef.insert(scanCoef.end(), blk, blk + nz);
                    slot.push_back(hdr.comp[c].first_block + (my * hdr.comp[c].vs + v) * hdr.comp[c].bw + mx * hdr.comp[c].hs + h);
                }
            }
            scanBegin.push_back((uint32_t)scanCoef.size());
            // de-interleave: per component, row-major
            std::vector<uint32_t> len(B);
            for (uint32_t i = 0; i < B; i++) len[slot[i]] = scanBegin[i + 1u] - scanBegin[i];
            out.begin.resize((size_t)B + 1u); out.begin[0] = 0u;
            for (uint32_t b = 0; b < B; b++) out.begin[b + 1u] = out.begin[b] + len[b];
            out.coef.resize(scanCoef.size());
            for (uint32_t i = 0; i < B; i++) std::memcpy(out.coef.data() + out.begin[slot[i]], scanCoef.data() + scanBegin[i], sizeof(int16_t) * (scanBegin[i + 1u] - scanBegin[i]));
            hdr.bytes = sizeof(zrjp::Header) + 4ull * ((uint64_t)B + 1u) + 2ull * out.coef.size();
            return out;
        }
        // (APPn, COM and every other segment with a length: skipped)
        at += len;
    }
}
// the record's bytes, padded with zeros to a multiple of 16 (hdr.bytes says where the record ends)
std::vector<uint8_t> JpegRecord(const JpegPacked& p)
{
    std::vector<uint8_t> r(((size_t)p.hdr.bytes + 15u) & ~(size_t)15u, 0);
    std::memcpy(r.data(), &p.hdr, sizeof(p.hdr));
    std::memcpy(r.data() + sizeof(p.hdr), p.begin.data(), 4u * p.begin.size());
    if (!p.coef.empty()) std::memcpy(r.data() + sizeof(p.hdr) + 4u * p.begin.size(), p.coef.data(), 2u * p.coef.size());
    return r;
}
// a checked record -> the texels of its channel map
std::vector<uint8_t> ExpandJpegRecord(const std::string& name, const uint8_t* rec, size_t bytes, zrjp::Header& h)
{
    if (const char* why = zrjp::CheckRecord(rec, bytes, &h)) Throw(name + ": invalid JPEG coefficient record: " + why);
    std::vector<uint8_t> planes(zrjp::PlaneBytes(h)), out((size_t)h.w * h.h * (h.map == (uint32_t)zrjp::kMapRgba ? 4u : 2u));
    zrjp::DecodeRecord(rec, h, planes.data(), out.data());
    return out;
}
// a .jpg image as the one-level Image of its slot: the texels of its channel map (default mode), or the record as `chain` (ZRH_LOAD_KEEP_COMPRESSED)
Image LoadJPEG(const std::string& path, bool colour, uint32_t map, bool keep)
{
    const std::vector<uint8_t> d = ReadFile(path);
    const std::vector<uint8_t> rec = JpegRecord(PackJpeg(path, d.data(), d.size(), map));
    zrjp::Header h;
    Image img; img.channels = colour ? 4 : 2; img.srgbFormat = colour;
    if (keep) { if (const char* why = zrjp::CheckRecord(rec.data(), rec.size(), &h)) Throw(path + ": invalid JPEG coefficient record: " + why); img.chain = rec; }
    else img.mip.push_back(ExpandJpegRecord(path, rec.data(), rec.size(), h));
    img.w = h.w; img.h = h.h;
    img.mips = 1; for (uint32_t m = h.w > h.h ? h.w : h.h; m > 1u; m >>= 1) img.mips++;
    return img;
}

} // namespace

struct zrh_scene_data
{
    std::vector<zr_vertex> vertices; std::vector<uint32_t> indices; std::vector<zr_mesh_instance> instances; std::vector<float> toWorld;
    std::vector<uint8_t> mask; std::vector<uint32_t> numTris; std::vector<zr_material> materials; std::vector<zr_emissive_triangle> emissives, emissivesInitial;
    std::vector<uint16_t> rho; uint32_t rhoDim[3] = {0, 0, 0};
    std::vector<zr_texture_desc> textures; std::vector<uint8_t> texels; uint32_t texOffsets[4] = {0, 0, 0, 0};
    // ZRH_LOAD_KEEP_COMPRESSED: `texels` stays empty; texSources[i] names the chain of textures[i] in texPayload, heapBytes is the size of the heap they decode to
    bool loadJpeg = false;      // ZRH_LOAD_JPEG
    bool deformedLights = false;      // ZRH_LOAD_DEFORMED_LIGHTS: a skinned or morphed primitive may carry an emissive material
    bool keepCompressed = false; std::vector<zr_texture_source> texSources; std::vector<uint8_t> texPayload; uint64_t heapBytes = 0; zr_texture_blocks blocks{};
    std::vector<float> prevWorld; uint32_t dirtyFirst = 0xffffffffu, dirtyEnd = 0;      // per-frame maintenance (zrh_scene_data_begin_frame / _set_instance_world)
    // the instances set_instance_world named this frame, each once, with their matrices; movedSlot[i] = where instance i stands in that list
    std::vector<uint32_t> movedIdx, movedSlot; std::vector<float> movedWorld;
    bool deviceRecords = false;      // zrh_scene_data_set_device_records (zr_host.h: zrh_scene_apply_updates)
    // keyframe animation (zrh_scene_data_set_animation: a deep copy; anim points into the vectors) and the node matrices of the last zrh_scene_data_animate
    std::vector<zr_anim_node> animNodes; std::vector<zr_keyframe> animKeys; std::vector<uint32_t> animInstIdx, animInstNode; std::vector<float> animWorld;
    zr_anim_desc anim{}; bool hasAnim = false, deviceAnimation = false;      // deviceAnimation: zrh_scene_data_set_device_animation (zr_host.h: zrh_scene_animate)
    // skinned meshes of the file (zrh_scene_data_skinning; skin points into the vectors): joints on entries of animNodes, one range per skinned primitive
    std::vector<zr_skin_joint> skinJoints; std::vector<zr_skin_range> skinRanges; std::vector<zr_skin_influence> skinInfluences;
    zr_skin_desc skin{}; bool hasSkin = false, deviceSkinning = false;      // deviceSkinning: zrh_scene_data_set_device_skinning (zr_host.h: zrh_scene_animate)
    std::vector<zr_vertex> skinRest, skinPosed;      // zrh_scene_data_skin_pose: the ranges' rest records (this scene's vertices, which keep the rest pose) and the posed ones
    // morph targets of the file (zrh_scene_data_morph; morph points into the vectors): one track per node with a weights channel, one range per primitive of such a node
    std::vector<zr_morph_track> morphTracks; std::vector<zr_morph_target> morphTargets; std::vector<zr_morph_range> morphRanges;
    std::vector<float> morphTimes, morphValues, morphRestWeights, morphDeltas;
    zr_morph_desc morph{}; bool hasMorph = false, deviceMorph = false;      // deviceMorph: zrh_scene_data_set_device_morph (zr_host.h: zrh_scene_animate)
    std::vector<zr_vertex> morphRest, morphPosed;      // zrh_scene_data_morph_pose
    std::vector<uint32_t> poseLights;      // zrh_scene_data_pose_lights
    void PointMorph()
    {
        std::memset(&morph, 0, sizeof(morph));
        morph.tracks = morphTracks.data(); morph.num_tracks = (uint32_t)morphTracks.size(); morph.targets = morphTargets.data(); morph.num_targets = (uint32_t)morphTargets.size();
        morph.ranges = morphRanges.data(); morph.num_ranges = (uint32_t)morphRanges.size(); morph.times = morphTimes.data(); morph.num_times = (uint32_t)morphTimes.size();
        morph.values = morphValues.data(); morph.num_values = (uint32_t)morphValues.size(); morph.rest_weights = morphRestWeights.data(); morph.num_rest_weights = (uint32_t)morphRestWeights.size();
        morph.deltas = morphDeltas.data(); morph.num_deltas = (uint32_t)(morphDeltas.size() / 3);
    }
    zr_scene_desc desc;
    void Finish()
    {
        std::memset(&desc, 0, sizeof(desc));
        desc.vertices = vertices.data(); desc.num_vertices = (uint32_t)vertices.size(); desc.indices = indices.data(); desc.num_indices = (uint32_t)indices.size();
        desc.instances = instances.data(); desc.num_instances = (uint32_t)instances.size(); desc.instance_to_world = toWorld.data();
        desc.instance_mask = mask.data(); desc.instance_num_tris = numTris.data(); desc.materials = materials.data(); desc.num_materials = (uint32_t)materials.size();
        desc.emissives = emissives.empty() ? nullptr : emissives.data(); desc.num_emissives = (uint32_t)emissives.size();
        desc.rho_lut = rho.data(); for (int k = 0; k < 3; k++) desc.rho_dim[k] = rhoDim[k];
        desc.textures = textures.empty() ? nullptr : textures.data(); desc.num_textures = (uint32_t)textures.size();
        desc.texels = texels.empty() ? nullptr : texels.data(); desc.texel_bytes = texels.size();
        if (keepCompressed && !texSources.empty()) { desc.texel_bytes = heapBytes; blocks.sources = texSources.data(); blocks.payload = texPayload.data(); blocks.payload_bytes = texPayload.size(); }
    }
};

namespace {

struct Accessor { const uint8_t* base; size_t stride; int comp, ncomp; size_t count; bool normalized; };
struct Gltf
{
    Json root; std::string dir; std::vector<std::vector<uint8_t>> buffers;
    Accessor Acc(int idx) const
    {
        // (indices as non-negative numbers below 2^32 before they become size_t: the conversion of a negative double is undefined)
        auto index = [](double v) -> size_t { if (!(v >= 0.0) || v >= 4294967296.0) Throw("glTF: accessor, bufferView or buffer index out of range"); return (size_t)v; };
        const Json& a = root.At("accessors").arr.at(index((double)idx));
        const Json& bv = root.At("bufferViews").arr.at(index(a.At("bufferView").num));
        const std::vector<uint8_t>& buf = buffers.at(index(bv.At("buffer").num));
        // (offsets, count and stride as non-negative numbers below 2^32: the size_t arithmetic below cannot wrap)
        for (double v : {a.At("count").num, a.NumOr("byteOffset", 0), bv.NumOr("byteOffset", 0), bv.NumOr("byteStride", 0)})
            if (!(v >= 0.0) || v >= 4294967296.0) Throw("glTF: accessor with a negative or oversized count, offset or stride");
        Accessor r; r.comp = (int)a.At("componentType").num; r.count = (size_t)a.At("count").num; r.normalized = a.BoolOr("normalized", false);
        const std::string t = a.At("type").str;
        r.ncomp = t == "SCALAR" ? 1 : t == "VEC2" ? 2 : t == "VEC3" ? 3 : t == "VEC4" ? 4 : t == "MAT4" ? 16 : 0;
        if (!r.ncomp) Throw("glTF: accessor type " + t + " is not supported");
        const size_t csz = (r.comp == 5120 || r.comp == 5121) ? 1 : (r.comp == 5122 || r.comp == 5123) ? 2 : 4;
        const size_t off = (size_t)bv.NumOr("byteOffset", 0) + (size_t)a.NumOr("byteOffset", 0);
        r.stride = (size_t)bv.NumOr("byteStride", 0); if (!r.stride) r.stride = csz * r.ncomp;
        if (off + (r.count ? (r.count - 1) * r.stride + csz * r.ncomp : 0) > buf.size()) Throw("glTF: accessor reads past its buffer");
        r.base = buf.data() + off;
        return r;
    }
    // `count` tightly packed elements of a bufferView, `byteOffset` into it: the parts of a sparse accessor (no accessor record of their own)
    Accessor View(double bufferView, double byteOffset, int comp, int ncomp, double count, bool normalized) const
    {
        for (double v : {bufferView, byteOffset, count}) if (!(v >= 0.0) || v >= 4294967296.0) Throw("glTF: sparse accessor with a negative or oversized count, offset or index");
        const Json& bv = root.At("bufferViews").arr.at((size_t)bufferView);
        const double bufIdx = bv.At("buffer").num, bvOff = bv.NumOr("byteOffset", 0);
        if (!(bufIdx >= 0.0) || bufIdx >= 4294967296.0 || !(bvOff >= 0.0) || bvOff >= 4294967296.0) Throw("glTF: accessor, bufferView or buffer index out of range");
        const std::vector<uint8_t>& buf = buffers.at((size_t)bufIdx);
        Accessor r; r.comp = comp; r.ncomp = ncomp; r.count = (size_t)count; r.normalized = normalized;
        const size_t csz = (comp == 5120 || comp == 5121) ? 1 : (comp == 5122 || comp == 5123) ? 2 : 4;
        const size_t off = (size_t)bvOff + (size_t)byteOffset;
        r.stride = csz * ncomp;
        if (off + r.count * r.stride > buf.size()) Throw("glTF: sparse accessor reads past its buffer");
        r.base = buf.data() + off;
        return r;
    }
    // a morph target's attribute: `nvtx` float triples from a VEC3 accessor of floats or normalised bytes / shorts, dense or SPARSE (sparse.indices /
    // sparse.values laid over the bufferView's elements, or over zeros without a bufferView -- the form exporters write deltas in); z negated like the vertices' z
    std::vector<float> Deltas(int idx, size_t nvtx, const std::string& where) const
    {
        if (idx < 0 || (size_t)idx >= root.At("accessors").Size()) Throw(where + "accessor index out of range");
        const Json& a = root.At("accessors").arr[(size_t)idx];
        const int comp = (int)a.At("componentType").num;
        const bool normalized = a.BoolOr("normalized", false);
        if (a.At("type").str != "VEC3" || !(comp == 5126 || ((comp == 5120 || comp == 5122 || comp == 5121 || comp == 5123) && normalized)))
            Throw(where + "a target attribute must be VEC3 of floats, or of normalised bytes / shorts");
        const double count = a.At("count").num;
        if (!(count >= 0.0) || count >= 4294967296.0) Throw("glTF: accessor with a negative or oversized count, offset or stride");
        if ((size_t)count < nvtx) Throw(where + "target accessor shorter than POSITION");
        std::vector<float> out(3 * nvtx, 0.0f);
        const Json* sp = a.Find("sparse");
        if (a.Find("bufferView"))
        {
            const Accessor d = Acc(idx);
            for (size_t v = 0; v < nvtx; v++) for (int c = 0; c < 3; c++) out[3 * v + c] = Comp(d, v, c);
        }
        else if (!sp) Throw(where + "a target accessor has neither a bufferView nor sparse data");
        if (sp)
        {
            const Json& si = sp->At("indices"); const Json& sv = sp->At("values");
            const int icomp = (int)si.At("componentType").num;
            if (icomp != 5121 && icomp != 5123 && icomp != 5125) Throw(where + "sparse indices must be unsigned bytes, shorts or ints");
            const Accessor ia = View(si.At("bufferView").num, si.NumOr("byteOffset", 0), icomp, 1, sp->At("count").num, false);
            const Accessor va = View(sv.At("bufferView").num, sv.NumOr("byteOffset", 0), comp, 3, sp->At("count").num, normalized);
            for (size_t k = 0; k < ia.count; k++)
            {
                const uint32_t i = Index(ia, k);
                if ((double)i >= count) Throw(where + "sparse index " + std::to_string(i) + " out of range: the accessor has " + std::to_string((size_t)count) + " elements");
                if (i < nvtx) for (int c = 0; c < 3; c++) out[3 * (size_t)i + c] = Comp(va, k, c);
            }
        }
        for (size_t v = 0; v < nvtx; v++) out[3 * v + 2] *= -1.0f;
        return out;
    }
    static float Comp(const Accessor& a, size_t i, int c)
    {
        const uint8_t* p = a.base + i * a.stride;
        switch (a.comp)
        {
        case 5126: { float f; std::memcpy(&f, p + 4 * c, 4); return f; }
        case 5121: { const float v = (float)p[c]; return a.normalized ? v / 255.0f : v; }
        case 5123: { uint16_t u; std::memcpy(&u, p + 2 * c, 2); return a.normalized ? (float)u / 65535.0f : (float)u; }
        case 5125: { uint32_t u; std::memcpy(&u, p + 4 * c, 4); return (float)u; }
        case 5120: { const float v = (float)(int8_t)p[c]; return a.normalized ? std::fmax(v / 127.0f, -1.0f) : v; }
        case 5122: { int16_t u; std::memcpy(&u, p + 2 * c, 2); return a.normalized ? std::fmax((float)u / 32767.0f, -1.0f) : (float)u; }
        default: Throw("glTF: unsupported component type");
        }
    }
    static uint32_t Index(const Accessor& a, size_t i)
    {
        const uint8_t* p = a.base + i * a.stride;
        if (a.comp == 5121) return p[0];
        if (a.comp == 5123) { uint16_t u; std::memcpy(&u, p, 2); return u; }
        if (a.comp == 5125) { uint32_t u; std::memcpy(&u, p, 4); return u; }
        Throw("glTF: index accessor must be unsigned");
    }
};

struct MeshPrim { uint32_t vtx, idx, nidx; int mat; uint32_t nvtx; };

void Load(const std::string& path, zrh_scene_data& sc)
{
    Gltf g;
    {   // the parser's strtod / strncmp look ahead: give them a NUL-terminated buffer (`end` stays at the last byte of the file)
        std::vector<uint8_t> txt = ReadFile(path); txt.push_back(0);
        JsonParser jp{(const char*)txt.data(), (const char*)txt.data() + txt.size() - 1}; g.root = jp.Value();
    }
    g.dir = DirOf(path);
    for (const Json& b : g.root.At("buffers").arr)
    {
        const std::string uri = b.StrOr("uri", "");
        if (uri.empty() || !uri.compare(0, 5, "data:")) Throw("glTF: only external .bin buffers are supported");
        g.buffers.push_back(ReadFile(g.dir + "/" + uri));
    }
    // ---- textures: one table per kind, heap = [base colour..., normal..., metallic-roughness..., emissive...] (the reference's four descriptor tables)
    std::vector<int> table[4]; std::map<int, uint32_t> slot[4];
    auto texSlot = [&](int kind, const Json* view) -> uint32_t {
        if (!view) return 0xffffu;
        const int texIdx = view->IntOr("index", -1); if (texIdx < 0) return 0xffffu;
        const int image = g.root.At("textures").arr.at(texIdx).IntOr("source", -1); if (image < 0) Throw("glTF: textureView doesn't point to any image");
        auto it = slot[kind].find(image); if (it != slot[kind].end()) return it->second;
        const uint32_t s = (uint32_t)table[kind].size(); table[kind].push_back(image); slot[kind][image] = s; return s; };
    // ---- materials (index 0 = the default material, glTF materials follow: MaterialIdx = glTF index + 1)
    { MaterialDesc d; d.metallic = 0.0f; d.roughness = 0.3f; sc.materials.push_back(PackMaterial(d)); }
    const Json* mats = g.root.Find("materials");
    for (size_t mi = 0; mats && mi < mats->Size(); mi++)
    {
        const Json& m = mats->arr[mi];
        MaterialDesc d;
        static const Json kEmpty;
        const Json& pbr = m.Find("pbrMetallicRoughness") ? *m.Find("pbrMetallicRoughness") : kEmpty;
        const Json& ext = m.Find("extensions") ? *m.Find("extensions") : kEmpty;
        if (const Json* f = pbr.Find("baseColorFactor")) for (int k = 0; k < 4; k++) d.baseColor[k] = (float)f->arr.at(k).num;
        d.metallic = (float)pbr.NumOr("metallicFactor", 1.0); d.roughness = (float)pbr.NumOr("roughnessFactor", 1.0);
        if (const Json* f = m.Find("emissiveFactor")) for (int k = 0; k < 3; k++) d.emissiveFactor[k] = (float)f->arr.at(k).num;
        if (const Json* e = ext.Find("KHR_materials_emissive_strength")) d.emissiveStrength = (float)e->NumOr("emissiveStrength", 1.0);
        if (const Json* e = ext.Find("KHR_materials_ior")) d.ior = (float)e->NumOr("ior", 1.5);
        if (const Json* e = ext.Find("KHR_materials_transmission")) d.transmission = (float)e->NumOr("transmissionFactor", 0.0);
        if (const Json* e = ext.Find("KHR_materials_clearcoat")) { d.coatWeight = (float)e->NumOr("clearcoatFactor", 0.0); d.coatRoughness = (float)e->NumOr("clearcoatRoughnessFactor", 0.0); }
        d.alphaCutoff = (float)m.NumOr("alphaCutoff", 0.5);
        const std::string am = m.StrOr("alphaMode", "OPAQUE"); d.alphaMode = am == "MASK" ? 1 : (am == "BLEND" ? 2 : 0);
        d.doubleSided = m.BoolOr("doubleSided", false);
        d.baseColorTex = texSlot(0, pbr.Find("baseColorTexture"));
        if (const Json* nt = m.Find("normalTexture")) { d.normalTex = texSlot(1, nt); d.normalScale = (float)nt->NumOr("scale", 1.0); }
        d.mrTex = texSlot(2, pbr.Find("metallicRoughnessTexture"));
        d.emissiveTex = texSlot(3, m.Find("emissiveTexture"));
        sc.materials.push_back(PackMaterial(d));
    }
    // decode the images into the texel heap
    for (int kind = 0; kind < 4; kind++)
    {
        sc.texOffsets[kind] = (uint32_t)sc.textures.size();
        for (int image : table[kind])
        {
            const std::string uri = g.root.At("images").arr.at(image).StrOr("uri", "");
            const bool png = EndsWith(uri, ".png");
            const bool jpeg = sc.loadJpeg && (EndsWith(uri, ".jpg") || EndsWith(uri, ".jpeg"));      // (ZRH_LOAD_JPEG; refused by name without it)
            if (!jpeg && (EndsWith(uri, ".jpg") || EndsWith(uri, ".jpeg"))) Throw("glTF: image '" + uri + "': JPEG images are not supported (.dds and .png are)");
            if (!png && !jpeg && !EndsWith(uri, ".dds")) Throw("glTF: image '" + uri + "': only .dds and .png images are supported");
            const bool colour = (kind == 0 || kind == 3);
            // a colour map keeps its BC7 blocks and an RG map its BC5 blocks: those decode straight to the heap's format.  Anything else (an RGBA8 file, a
            // 4-channel file in an RG slot) is decoded here as in the default mode and travels as a RAW chain.
            // A .png is level 0 alone: RGBA8 for a colour map, the file's (R, G) for a normal map and its (B, G) for a metallic-roughness map (glTF keeps
            // roughness in G and metalness in B; the reference's converter moves them to (metalness, roughness) with -swizzle bg).  Its full chain,
            // 1 + floor(log2(max(w, h))) levels, is generated by include/zr_mipgen.h: here (default mode), or on the device from a RAW_MIP0 source
            // A .jpg is level 0 alone too, with the same slots and chain: decoded here through include/zr_jpeg.h (default mode), or handed over as the
            // record of its entropy-decoded coefficients (a JPEG_COEF source), which the same header turns into level 0 on the device
            const Image img = jpeg ? LoadJPEG(g.dir + "/" + uri, colour, colour ? (uint32_t)zrjp::kMapRgba : (kind == 2 ? (uint32_t)zrjp::kMapBg : (uint32_t)zrjp::kMapRg), sc.keepCompressed)
                            : png ? LoadPNG(g.dir + "/" + uri, colour, kind == 2 ? 2u : 0u, 1u)
                                  : LoadDDS(g.dir + "/" + uri, !sc.keepCompressed ? ZR_TEX_SRC_RAW : (colour ? ZR_TEX_SRC_BC7 : ZR_TEX_SRC_BC5));
            if (colour && img.channels != 4) Throw(uri + ": base colour / emissive maps must be 4-channel");
            zr_texture_desc td; std::memset(&td, 0, sizeof(td));
            // (in the compressed mode the heap's texels are written here too, into a scratch vector that becomes the RAW chain)
            std::vector<uint8_t> raw; std::vector<uint8_t>& texels = sc.keepCompressed ? raw : sc.texels;
            if (!sc.keepCompressed) while (sc.texels.size() & 3) sc.texels.push_back(0);
            else sc.heapBytes = (sc.heapBytes + 3u) & ~(uint64_t)3u;
            td.offset = sc.keepCompressed ? sc.heapBytes : (uint64_t)sc.texels.size(); td.width = (uint16_t)img.w; td.height = (uint16_t)img.h; td.num_mips = (uint8_t)img.mips;
            td.format = colour ? ZR_TEX_RGBA8_SRGB : ZR_TEX_RG8;
            for (const auto& mp : img.mip)
            {
                if (!colour && img.channels == 4) { for (size_t i = 0; i < mp.size(); i += 4) { texels.push_back(mp[i]); texels.push_back(mp[i + 1]); } }      // RGBA8 normal / MR map: keep RG
                else texels.insert(texels.end(), mp.begin(), mp.end());
            }
            if ((png || jpeg) && !sc.keepCompressed)
            {   // the other levels, from level 0 in place
                const zr_tex_mip last = zr_tex_mip_of(&td, td.num_mips - 1u);
                sc.texels.resize(last.offset + (size_t)last.w * last.h * (colour ? 4u : 2u));
                zrmg::GenerateChain(&td, sc.texels.data());
            }
            if (sc.keepCompressed)
            {
                zr_texture_source src; std::memset(&src, 0, sizeof(src));
                while (sc.texPayload.size() & 15) sc.texPayload.push_back(0);
                src.offset = sc.texPayload.size(); src.encoding = jpeg ? (uint8_t)ZR_TEX_SRC_JPEG_COEF : png ? (uint8_t)ZR_TEX_SRC_RAW_MIP0 : img.chain.empty() ? (uint8_t)ZR_TEX_SRC_RAW : (uint8_t)(colour ? ZR_TEX_SRC_BC7 : ZR_TEX_SRC_BC5);
                const std::vector<uint8_t>& chain = img.chain.empty() ? raw : img.chain;
                sc.texPayload.insert(sc.texPayload.end(), chain.begin(), chain.end());
                const zr_tex_mip last = zr_tex_mip_of(&td, td.num_mips - 1u);
                sc.heapBytes = last.offset + (uint64_t)last.w * last.h * (colour ? 4u : 2u);
                sc.texSources.push_back(src);
            }
            sc.textures.push_back(td);
        }
    }
    // ---- meshes: one entry per (mesh, primitive); RH -> LH: z flipped, winding swapped (glTF.cpp:163-236)
    std::map<std::pair<int, int>, MeshPrim> prims;
    const Json& meshes = g.root.At("meshes");
    for (size_t mi = 0; mi < meshes.Size(); mi++)
    {
        const Json& plist = meshes.arr[mi].At("primitives");
        for (size_t pi = 0; pi < plist.Size(); pi++)
        {
            const Json& prim = plist.arr[pi];
            if (prim.IntOr("mode", 4) != 4) Throw("glTF: only triangle-list primitives are supported");
            const Json& at = prim.At("attributes");
            if (!at.Find("POSITION")) Throw("POSITION was not found in the vertex attributes.");
            if (!at.Find("NORMAL")) Throw("NORMAL was not found in the vertex attributes.");
            const Accessor pos = g.Acc((int)at.At("POSITION").num), nrm = g.Acc((int)at.At("NORMAL").num);
            MeshPrim mp; mp.vtx = (uint32_t)sc.vertices.size(); mp.idx = (uint32_t)sc.indices.size(); mp.mat = prim.IntOr("material", -1);
            const bool hasUV = at.Find("TEXCOORD_0") != nullptr, hasTan = hasUV && at.Find("TANGENT") != nullptr;
            Accessor uv{}, tan{};
            if (hasUV) uv = g.Acc((int)at.At("TEXCOORD_0").num);
            if (hasTan) tan = g.Acc((int)at.At("TANGENT").num);
            // every attribute is read for pos.count vertices: each accessor must hold that many elements
            if (nrm.count < pos.count || (hasUV && uv.count < pos.count) || (hasTan && tan.count < pos.count))
                Throw("glTF: NORMAL / TEXCOORD_0 / TANGENT accessor shorter than POSITION");
            const int numMats = mats ? (int)mats->Size() : 0;
            if (mp.mat >= numMats) Throw("glTF: primitive names material " + std::to_string(mp.mat) + " but the file has " + std::to_string(numMats));
            for (size_t v = 0; v < pos.count; v++)
            {
                zr_vertex vx; std::memset(&vx, 0, sizeof(vx));
                const float n[3] = {Gltf::Comp(nrm, v, 0), Gltf::Comp(nrm, v, 1), Gltf::Comp(nrm, v, 2) * -1.0f};
                vx.pos[0] = Gltf::Comp(pos, v, 0); vx.pos[1] = Gltf::Comp(pos, v, 1); vx.pos[2] = Gltf::Comp(pos, v, 2) * -1.0f;
                EncodeOct32(n, vx.normal);
                if (hasUV) { vx.uv[0] = Gltf::Comp(uv, v, 0); vx.uv[1] = Gltf::Comp(uv, v, 1); }
                if (hasTan) { const float t[3] = {Gltf::Comp(tan, v, 0), Gltf::Comp(tan, v, 1), Gltf::Comp(tan, v, 2) * -1.0f}; EncodeOct32(t, vx.tangent); }
                sc.vertices.push_back(vx);
            }
            if (!prim.Find("indices")) Throw("glTF: non-indexed primitives are not supported");
            const Accessor ia = g.Acc((int)prim.At("indices").num);
            if (ia.count % 3) Throw("glTF: index count is not a multiple of 3");
            for (size_t t = 0; t < ia.count; t += 3)
            {
                const uint32_t i0 = Gltf::Index(ia, t), i1 = Gltf::Index(ia, t + 2), i2 = Gltf::Index(ia, t + 1);
                // an index beyond the primitive's vertices would read past the vertex buffer on the host and on the device (BVH build, refit)
                if (i0 >= pos.count || i1 >= pos.count || i2 >= pos.count) Throw("glTF: vertex index out of range");
                sc.indices.push_back(i0); sc.indices.push_back(i1); sc.indices.push_back(i2);
            }
            mp.nidx = (uint32_t)ia.count; mp.nvtx = (uint32_t)pos.count;
            prims[{(int)mi, (int)pi}] = mp;
        }
    }
    // ---- morph targets: how many every mesh has (all primitives of a mesh alike: the node's weights drive them together) and its default weights
    std::vector<uint32_t> meshTargets(meshes.Size(), 0);
    std::vector<std::vector<float>> meshWeights(meshes.Size());
    for (size_t mi = 0; mi < meshes.Size(); mi++)
    {
        const Json& plist = meshes.arr[mi].At("primitives");
        const std::string where = "glTF: mesh " + std::to_string(mi) + " ('" + meshes.arr[mi].StrOr("name", "") + "'): ";
        for (size_t pi = 0; pi < plist.Size(); pi++)
        {
            const Json* tg = plist.arr[pi].Find("targets");
            const uint32_t n = tg ? (uint32_t)tg->Size() : 0u;
            if (pi && n != meshTargets[mi]) Throw(where + "its primitives have different morph target counts (" + std::to_string(meshTargets[mi]) + " and " + std::to_string(n) + ")");
            meshTargets[mi] = n;
        }
        if (!meshTargets[mi]) continue;
        meshWeights[mi].assign(meshTargets[mi], 0.0f);
        if (const Json* w = meshes.arr[mi].Find("weights"))
        {
            if (w->Size() != meshTargets[mi]) Throw(where + "a weights array of " + std::to_string(w->Size()) + " entries, the mesh has " + std::to_string(meshTargets[mi]) + " morph targets");
            for (uint32_t k = 0; k < meshTargets[mi]; k++) meshWeights[mi][k] = (float)w->arr[k].num;
        }
    }
    // ---- nodes, depth first: world = local x parent (SceneCore.cpp:871-873); one instance per primitive
    struct Em { uint32_t inst; MeshPrim mp; };
    std::vector<Em> emissive;
    const Json& nodes = g.root.At("nodes");
    auto isEmissive = [&](int mat) {
        if (mat < 0 || !mats) return false;
        const Json& m = mats->arr.at(mat);
        float sum = 0; if (const Json* f = m.Find("emissiveFactor")) sum = (float)f->arr.at(0).num + (float)f->arr.at(1).num + (float)f->arr.at(2).num;
        // glTF.cpp:405-410: factor sum > 0 OR KHR_materials_emissive_strength present OR an emissive texture
        bool hasStrength = false;
        if (const Json* ext = m.Find("extensions")) hasStrength = ext->Find("KHR_materials_emissive_strength") != nullptr;
        return sum > 0 || hasStrength || m.Find("emissiveTexture") != nullptr; };
    Mat43 identity; std::memset(&identity, 0, sizeof(identity)); for (int i = 0; i < 3; i++) identity.m[i][i] = 1.0f;
    // ---- "animations": per animated node the input accessor its channels share and one output accessor per path (-1: the node's rest value at every
    // key).  LINEAR samplers on translation / rotation / scale only; anything else fails the load with the animation and the node named
    struct NodeAnim { int input = -1, out[3] = {-1, -1, -1}; std::string anim; };      // out: translation, rotation, scale
    std::map<int, NodeAnim> nodeAnims;
    // ... and per node with a `weights` channel (LINEAR; the output a SCALAR accessor of keys x targets) its sampler's accessors
    struct WeightAnim { int input = -1, output = -1; std::string anim; };
    std::map<int, WeightAnim> weightAnims;
    if (const Json* anims = g.root.Find("animations"))
        for (size_t ai = 0; ai < anims->Size(); ai++)
        {
            const Json& a = anims->arr[ai];
            const std::string aname = "animation " + std::to_string(ai) + " ('" + a.StrOr("name", "") + "')";
            const Json& samplers = a.At("samplers");
            for (const Json& ch : a.At("channels").arr)
            {
                const Json& target = ch.At("target");
                const int node = target.IntOr("node", -1);
                if (node < 0) continue;      // (a channel without a target node is ignored, as the specification says)
                const std::string where = "glTF: " + aname + ", node " + std::to_string(node) + ": ";
                if ((size_t)node >= nodes.arr.size()) Throw(where + "node index out of range");
                const std::string path = target.StrOr("path", "");
                if (path == "weights")
                {
                    const int mesh = nodes.arr[(size_t)node].IntOr("mesh", -1);
                    const uint32_t T = mesh >= 0 && (size_t)mesh < meshTargets.size() ? meshTargets[(size_t)mesh] : 0u;
                    if (!T) Throw(where + "target path 'weights': the node's mesh has no morph targets");
                    const Json& sm = samplers.arr.at((size_t)ch.At("sampler").num);
                    const std::string interp = sm.StrOr("interpolation", "LINEAR");
                    if (interp != "LINEAR") Throw(where + "target path 'weights': " + interp + " samplers are not supported (LINEAR is)");
                    if (weightAnims.count(node)) Throw(where + "two channels target its weights");
                    WeightAnim wa; wa.input = (int)sm.At("input").num; wa.output = (int)sm.At("output").num; wa.anim = aname;
                    const Accessor in = g.Acc(wa.input), out = g.Acc(wa.output);
                    if (in.count < 2) Throw(where + "target path 'weights': fewer than 2 keys");
                    if (in.ncomp != 1 || out.ncomp != 1 || out.count < in.count * T) Throw(where + "sampler accessors do not match the weights path (a SCALAR output of keys x " + std::to_string(T) + " targets)");
                    weightAnims[node] = wa;
                    continue;
                }
                const int which = path == "translation" ? 0 : path == "rotation" ? 1 : path == "scale" ? 2 : -1;
                if (which < 0) Throw(where + "target path '" + path + "' is not supported (translation, rotation and scale are)");
                const Json& sm = samplers.arr.at((size_t)ch.At("sampler").num);
                const std::string interp = sm.StrOr("interpolation", "LINEAR");
                if (interp != "LINEAR") Throw(where + interp + " samplers are not supported (LINEAR is)");
                NodeAnim& na = nodeAnims[node];
                const int input = (int)sm.At("input").num;
                if (na.input >= 0 && na.input != input) Throw(where + "its channels use different input accessors (per-channel key times are not supported)");
                if (na.out[which] >= 0) Throw(where + "two channels target its " + path);
                na.input = input; na.out[which] = (int)sm.At("output").num; na.anim = aname;
                const Accessor in = g.Acc(input), out = g.Acc(na.out[which]);
                if (in.count < 2) Throw(where + "fewer than 2 keys");
                if (out.count < in.count || out.ncomp != (which == 1 ? 4 : 3) || in.ncomp != 1) Throw(where + "sampler accessors do not match the " + path + " path");
            }
        }
    // ---- "skins": the joints (nodes of the file) and inverse bind matrices of every skin a node with a mesh uses.  The matrices take the loader's
    // handedness rule for node matrices (z row and z column negated: S M S with S = diag(1, 1, -1), what negating a translation's z and a rotation's x
    // and y is), so that J = world x inverse bind acts on the z-negated vertices as the file's J acts on the file's
    struct SkinUse { std::vector<int> joints; std::vector<float> ibm; std::string name; bool used = false; uint32_t base = 0; };
    std::vector<SkinUse> skins;
    if (const Json* sk = g.root.Find("skins"))
        for (size_t si = 0; si < sk->Size(); si++)
        {
            SkinUse u; u.name = "glTF: skin " + std::to_string(si) + " ('" + sk->arr[si].StrOr("name", "") + "'): ";
            for (const Json& j : sk->arr[si].At("joints").arr)
            {
                if (!(j.num >= 0) || j.num >= (double)nodes.arr.size()) Throw(u.name + "joint " + std::to_string(u.joints.size()) + " is not a node of the file");
                u.joints.push_back((int)j.num);
            }
            if (u.joints.empty()) Throw(u.name + "no joints");
            if (u.joints.size() > 65535) Throw(u.name + "more than 65 535 joints");
            u.ibm.assign(12 * u.joints.size(), 0.0f);
            for (size_t j = 0; j < u.joints.size(); j++) u.ibm[12 * j] = u.ibm[12 * j + 5] = u.ibm[12 * j + 10] = 1.0f;
            const int ibmAcc = sk->arr[si].IntOr("inverseBindMatrices", -1);
            if (ibmAcc >= 0)
            {
                const Accessor a = g.Acc(ibmAcc);
                if (a.ncomp != 16 || a.comp != 5126 || a.count < u.joints.size()) Throw(u.name + "inverseBindMatrices must be a float MAT4 accessor with one matrix per joint");
                for (size_t j = 0; j < u.joints.size(); j++)
                {
                    Mat43 r; for (int i = 0; i < 4; i++) for (int c = 0; c < 3; c++) r.m[i][c] = Gltf::Comp(a, j, 4 * i + c);
                    r.m[0][2] *= -1.0f; r.m[1][2] *= -1.0f; r.m[2][0] *= -1.0f; r.m[2][1] *= -1.0f; r.m[3][2] *= -1.0f;
                    ToToWorld(r, u.ibm.data() + 12 * j);
                }
            }
            skins.push_back(std::move(u));
        }
    for (const Json& n : nodes.arr)
    {
        const int s = n.IntOr("skin", -1);
        if (s < 0 || n.IntOr("mesh", -1) < 0) continue;
        if ((size_t)s >= skins.size()) Throw("glTF: a node names skin " + std::to_string(s) + " but the file has " + std::to_string(skins.size()));
        skins[(size_t)s].used = true;
    }
    // is the node a joint of a used skin, or an ancestor of one?  (the dynamic closure keeps those: their world matrices feed the joint matrices)
    std::vector<int8_t> leadsToJoint(nodes.arr.size(), -1);
    std::vector<uint8_t> isJoint(nodes.arr.size(), 0);
    for (const SkinUse& u : skins) if (u.used) for (int j : u.joints) isJoint[(size_t)j] = 1;
    std::vector<uint32_t> nodeEntry(nodes.arr.size(), ZR_ANIM_ROOT);      // a visited node's entry of the closure table
    struct SkinnedPrim { int skin; uint32_t range; };
    std::vector<SkinnedPrim> skinnedPrims;
    // does the subtree of a node hold a mesh?  (a descendant of an animated node joins the closure only if it carries, or leads to, an instance)
    std::vector<int8_t> leadsToMesh(nodes.arr.size(), -1);
    struct Walker
    {
        Gltf& g; zrh_scene_data& sc; std::map<std::pair<int, int>, MeshPrim>& prims; std::vector<Em>& emissive; const Json& nodes; decltype(isEmissive)& isEm;
        std::vector<uint8_t> onPath;
        std::map<int, NodeAnim>& nodeAnims; std::vector<int8_t>& leadsToMesh;
        std::vector<SkinUse>& skins; std::vector<int8_t>& leadsToJoint; std::vector<uint8_t>& isJoint; std::vector<uint32_t>& nodeEntry; std::vector<SkinnedPrim>& skinnedPrims;
        std::vector<uint32_t>& meshTargets; std::vector<std::vector<float>>& meshWeights; std::map<int, WeightAnim>& weightAnims;
        std::map<std::pair<int, int>, uint32_t> primTargets;      // (mesh, primitive) -> its first entry of the target table: nodes that share a mesh share its deltas
        // a copy of the primitive's vertices as a range of its own (nothing is shared with another node that uses the mesh); returns its first vertex
        uint32_t CopyPrimitive(const MeshPrim& mp)
        {
            const uint32_t first = (uint32_t)sc.vertices.size();
            for (uint32_t v = 0; v < mp.nvtx; v++) sc.vertices.push_back(sc.vertices[mp.vtx + v]);
            return first;
        }
        // the targets of one primitive in the target table and the delta pool (read once per mesh primitive); returns the first entry
        uint32_t PrimTargets(int mesh, int pi, const Json& prim, const MeshPrim& mp, const std::string& where)
        {
            const auto it = primTargets.find({mesh, pi});
            if (it != primTargets.end()) return it->second;
            const uint32_t first = (uint32_t)sc.morphTargets.size();
            const Json& tg = prim.At("targets");
            for (size_t k = 0; k < tg.Size(); k++)
            {
                zr_morph_target m; m.first_pos = m.first_nrm = m.first_tan = ZR_MORPH_NONE;
                uint32_t* firsts[3] = {&m.first_pos, &m.first_nrm, &m.first_tan};
                const char* names[3] = {"POSITION", "NORMAL", "TANGENT"};
                for (int a = 0; a < 3; a++)
                    if (const Json* acc = tg.arr[k].Find(names[a]))
                    {
                        const std::vector<float> d = g.Deltas((int)acc->num, mp.nvtx, where + "target " + std::to_string(k) + " " + names[a] + ": ");
                        *firsts[a] = (uint32_t)(sc.morphDeltas.size() / 3);
                        sc.morphDeltas.insert(sc.morphDeltas.end(), d.begin(), d.end());
                    }
                sc.morphTargets.push_back(m);
            }
            primTargets[{mesh, pi}] = first;
            return first;
        }
        // one primitive of a node whose mesh has morph targets, its vertices a range of the node's own at `first`.  With a weights channel (track >= 0): a
        // morph range under the node's track.  Without: the default weights are applied here, once, by zrmo::MorphVertex, and no range is listed
        void MorphPrimitive(int nidx, int mesh, int pi, const Json& prim, const MeshPrim& mp, uint32_t first, int track, const std::vector<float>& weights)
        {
            const std::string where = "glTF: node " + std::to_string(nidx) + " (mesh " + std::to_string(mesh) + ", primitive " + std::to_string(pi) + "): ";
            if (isEm(mp.mat) && !sc.deformedLights) Throw(where + "a morphed primitive with an emissive material is not supported (a deformed light would keep shining from its rest pose)");
            const uint32_t T = meshTargets[(size_t)mesh];
            if (track >= 0)
            {
                const uint32_t firstTarget = PrimTargets(mesh, pi, prim, mp, where);
                sc.morphRanges.push_back(zr_morph_range{first, mp.nvtx, firstTarget, T, (uint32_t)track});
                return;
            }
            bool any = false; for (float w : weights) { if (!Finite(w)) Throw(where + "a default weight is not finite"); any = any || w != 0.0f; }
            if (!any) return;
            // (the baked mesh's targets go to a table of their own: nothing of them stays in the scene)
            std::vector<zr_morph_target> table; std::vector<float> pool;
            const Json& tg = prim.At("targets");
            for (size_t k = 0; k < tg.Size(); k++)
            {
                zr_morph_target m; m.first_pos = m.first_nrm = m.first_tan = ZR_MORPH_NONE;
                uint32_t* firsts[3] = {&m.first_pos, &m.first_nrm, &m.first_tan};
                const char* names[3] = {"POSITION", "NORMAL", "TANGENT"};
                for (int a = 0; a < 3; a++)
                    if (const Json* acc = tg.arr[k].Find(names[a]))
                    {
                        const std::vector<float> d = g.Deltas((int)acc->num, mp.nvtx, where + "target " + std::to_string(k) + " " + names[a] + ": ");
                        for (float x : d) if (!Finite(x)) Throw(where + "target " + std::to_string(k) + ": a delta is not finite");
                        *firsts[a] = (uint32_t)(pool.size() / 3);
                        pool.insert(pool.end(), d.begin(), d.end());
                    }
                table.push_back(m);
            }
            for (uint32_t v = 0; v < mp.nvtx; v++)
            {
                const zr_vertex rest = sc.vertices[first + v];
                zrmo::MorphVertex(rest, table.data(), T, weights.data(), pool.data(), v, sc.vertices[first + v]);
            }
        }
        bool LeadsToJoint(int nidx, int depth = 0)
        {
            if (nidx < 0 || (size_t)nidx >= nodes.arr.size() || depth > 4096) return false;
            if (leadsToJoint[nidx] >= 0) return leadsToJoint[nidx] != 0;
            leadsToJoint[nidx] = 0;      // (a cycle ends here; Visit names it)
            const Json& node = nodes.arr.at(nidx);
            bool any = isJoint[nidx] != 0;
            if (const Json* ch = node.Find("children")) for (const Json& c : ch->arr) any = LeadsToJoint((int)c.num, depth + 1) || any;
            leadsToJoint[nidx] = any ? 1 : 0;
            return any;
        }
        // one primitive of a skinned node: a vertex range of its own (a copy of the mesh's: no sharing with another node that uses the mesh), its influences
        // (JOINTS_0: unsigned bytes or shorts; WEIGHTS_0: floats, or normalised bytes / shorts; renormalised to sum 1 in float32).  Returns the copy's first vertex
        uint32_t SkinPrimitive(int nidx, int skin, const Json& prim, const MeshPrim& mp)
        {
            const std::string where = "glTF: node " + std::to_string(nidx) + " (skin " + std::to_string(skin) + "): ";
            const Json& at = prim.At("attributes");
            if (at.Find("JOINTS_1") || at.Find("WEIGHTS_1")) Throw(where + "JOINTS_1 / WEIGHTS_1: more than four influences per vertex are not supported");
            const bool hj = at.Find("JOINTS_0") != nullptr, hw = at.Find("WEIGHTS_0") != nullptr;
            if (hj && !hw) Throw(where + "JOINTS_0 without WEIGHTS_0");
            if (hw && !hj) Throw(where + "WEIGHTS_0 without JOINTS_0");
            if (!hj) Throw(where + "a primitive of a skinned node has neither JOINTS_0 nor WEIGHTS_0");
            if (isEm(mp.mat) && !sc.deformedLights) Throw(where + "a skinned primitive with an emissive material is not supported (a deformed light would keep shining from its rest pose)");
            const Accessor ja = g.Acc((int)at.At("JOINTS_0").num), wa = g.Acc((int)at.At("WEIGHTS_0").num);
            if (ja.ncomp != 4 || (ja.comp != 5121 && ja.comp != 5123) || ja.normalized) Throw(where + "JOINTS_0 must be VEC4 of unsigned bytes or unsigned shorts");
            if (wa.ncomp != 4 || !(wa.comp == 5126 || ((wa.comp == 5121 || wa.comp == 5123) && wa.normalized))) Throw(where + "WEIGHTS_0 must be VEC4 of floats, or of normalised unsigned bytes / shorts");
            if (ja.count < mp.nvtx || wa.count < mp.nvtx) Throw(where + "JOINTS_0 / WEIGHTS_0 accessor shorter than POSITION");
            const size_t numJoints = skins[(size_t)skin].joints.size();
            const uint32_t first = (uint32_t)sc.vertices.size();
            zr_skin_range range; range.first_vertex = first; range.num_vertices = mp.nvtx; range.first_influence = (uint32_t)sc.skinInfluences.size();
            for (uint32_t v = 0; v < mp.nvtx; v++)
            {
                sc.vertices.push_back(sc.vertices[mp.vtx + v]);
                zr_skin_influence f; float w[4];
                for (int k = 0; k < 4; k++)
                {
                    const uint32_t j = (uint32_t)Gltf::Comp(ja, v, k);
                    if (j >= numJoints) Throw(where + "vertex " + std::to_string(v) + ": joint " + std::to_string(j) + ", the skin has " + std::to_string(numJoints));
                    f.joint[k] = (uint16_t)j; w[k] = Gltf::Comp(wa, v, k);
                }
                const float sum = ((w[0] + w[1]) + w[2]) + w[3];
                if (!(sum > 0.0f) || !Finite(sum)) Throw(where + "vertex " + std::to_string(v) + ": the weights do not sum to a positive finite number");
                for (int k = 0; k < 4; k++) f.weight[k] = w[k] / sum;
                sc.skinInfluences.push_back(f);
            }
            skinnedPrims.push_back(SkinnedPrim{skin, (uint32_t)sc.skinRanges.size()});
            sc.skinRanges.push_back(range);
            return first;
        }
        bool LeadsToMesh(int nidx, int depth = 0)
        {
            if (nidx < 0 || (size_t)nidx >= nodes.arr.size() || depth > 4096) return false;
            if (leadsToMesh[nidx] >= 0) return leadsToMesh[nidx] != 0;
            const Json& node = nodes.arr.at(nidx);
            bool any = node.IntOr("mesh", -1) >= 0;
            if (const Json* ch = node.Find("children")) for (const Json& c : ch->arr) any = LeadsToMesh((int)c.num, depth + 1) || any;
            leadsToMesh[nidx] = any ? 1 : 0;
            return any;
        }
        // closureParent: the node's parent in the closure table, ZR_ANIM_ROOT when no ancestor is animated
        void Visit(int nidx, const Mat43& parent, uint32_t closureParent = ZR_ANIM_ROOT)
        {
            if (nidx < 0 || (size_t)nidx >= nodes.arr.size()) Throw("glTF: node index out of range");
            if (onPath.empty()) onPath.assign(nodes.arr.size(), 0);
            if (onPath[nidx]) Throw("glTF: the node hierarchy has a cycle");
            onPath[nidx] = 1;
            struct Leave { std::vector<uint8_t>& v; int i; ~Leave() { v[i] = 0; } } leave{onPath, nidx};
            const Json& node = nodes.arr.at(nidx);
            float s[3] = {1, 1, 1}, q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
            if (const Json* m = node.Find("matrix"))
            {
                // column-major glTF matrix -> row-vector rows; RH -> LH (glTF.cpp:800-833), then decomposed like the reference's decomposeTRS
                float M[16]; for (int k = 0; k < 16; k++) M[k] = (float)m->arr.at(k).num;
                Mat43 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 3; j++) r.m[i][j] = M[4 * i + j];
                r.m[0][2] *= -1.0f; r.m[1][2] *= -1.0f; r.m[2][0] *= -1.0f; r.m[2][1] *= -1.0f; r.m[3][2] *= -1.0f;
                DecomposeSRT(r, s, q, t);
            }
            else
            {
                if (const Json* a = node.Find("scale")) for (int k = 0; k < 3; k++) { s[k] = (float)a->arr.at(k).num; if (!(s[k] > 0)) Throw("Negative scale factors are not supported."); }
                if (const Json* a = node.Find("translation")) { t[0] = (float)a->arr.at(0).num; t[1] = (float)a->arr.at(1).num; t[2] = (float)-a->arr.at(2).num; }
                if (const Json* a = node.Find("rotation")) { q[0] = -(float)a->arr.at(0).num; q[1] = -(float)a->arr.at(1).num; q[2] = (float)a->arr.at(2).num; q[3] = (float)a->arr.at(3).num; }
            }
            const Mat43 world = Mul(AffineTransformation(s, q, t), parent);
            // ---- the dynamic closure, depth first (a parent precedes its children): the animated nodes and what hangs on them
            uint32_t entry = ZR_ANIM_ROOT;
            const auto anim = nodeAnims.find(nidx);
            const int meshOfNode = node.IntOr("mesh", -1);
            const bool morphed = meshOfNode >= 0 && (size_t)meshOfNode < meshTargets.size() && meshTargets[(size_t)meshOfNode] > 0;
            const auto wanim = morphed ? weightAnims.find(nidx) : weightAnims.end();
            // (a node whose weights are animated joins the closure even when no transform of it is: a file whose only animation is a weights channel has an animation to set)
            if (anim != nodeAnims.end() || (closureParent != ZR_ANIM_ROOT && LeadsToMesh(nidx)) || LeadsToJoint(nidx) || wanim != weightAnims.end())
            {
                zr_anim_node an; std::memset(&an, 0, sizeof(an));
                an.parent = closureParent;
                for (int k = 0; k < 3; k++) { an.rest_scale[k] = s[k]; an.rest_translation[k] = t[k]; }
                for (int k = 0; k < 4; k++) an.rest_rotation[k] = q[k];
                if (closureParent == ZR_ANIM_ROOT) ToToWorld(parent, an.parent_world);      // the static world matrix above the node (unused below a closure node)
                if (anim != nodeAnims.end())
                {
                    const NodeAnim& na = anim->second;
                    const Accessor in = g.Acc(na.input);
                    an.first_key = (uint32_t)sc.animKeys.size(); an.num_keys = (uint32_t)in.count; an.loop = 1; an.t0 = 0.0f;
                    Accessor out[3]; for (int w = 0; w < 3; w++) if (na.out[w] >= 0) out[w] = g.Acc(na.out[w]);
                    for (size_t k = 0; k < in.count; k++)
                    {
                        // the node's own handedness conversion: translation z negated, rotation x and y negated
                        zr_keyframe key; std::memset(&key, 0, sizeof(key));
                        key.time = Gltf::Comp(in, k, 0);
                        for (int c = 0; c < 3; c++) { key.scale[c] = s[c]; key.translation[c] = t[c]; }
                        for (int c = 0; c < 4; c++) key.rotation[c] = q[c];
                        if (na.out[0] >= 0) { key.translation[0] = Gltf::Comp(out[0], k, 0); key.translation[1] = Gltf::Comp(out[0], k, 1); key.translation[2] = -Gltf::Comp(out[0], k, 2); }
                        if (na.out[1] >= 0) { key.rotation[0] = -Gltf::Comp(out[1], k, 0); key.rotation[1] = -Gltf::Comp(out[1], k, 1); key.rotation[2] = Gltf::Comp(out[1], k, 2); key.rotation[3] = Gltf::Comp(out[1], k, 3); }
                        if (na.out[2] >= 0) for (int c = 0; c < 3; c++) { key.scale[c] = Gltf::Comp(out[2], k, c); if (!(key.scale[c] > 0)) Throw("glTF: " + na.anim + ", node " + std::to_string(nidx) + ": negative scale factors are not supported"); }
                        sc.animKeys.push_back(key);
                    }
                }
                entry = (uint32_t)sc.animNodes.size();
                sc.animNodes.push_back(an);
                nodeEntry[nidx] = entry;
            }
            const int mesh = node.IntOr("mesh", -1);
            const int skin = mesh >= 0 ? node.IntOr("skin", -1) : -1;      // a skinned node: glTF ignores its own transform, the joints place the mesh
            int track = -1;
            std::vector<float> nodeWeights;
            if (morphed)
            {   // the node's weights (its own override the mesh's), and its track when a channel drives them
                const uint32_t T = meshTargets[(size_t)mesh];
                nodeWeights = meshWeights[(size_t)mesh];
                if (const Json* w = node.Find("weights"))
                {
                    if (w->Size() != T) Throw("glTF: node " + std::to_string(nidx) + ": a weights array of " + std::to_string(w->Size()) + " entries, its mesh has " + std::to_string(T) + " morph targets");
                    for (uint32_t k = 0; k < T; k++) nodeWeights[k] = (float)w->arr[k].num;
                }
                if (wanim != weightAnims.end())
                {
                    const Accessor in = g.Acc(wanim->second.input), out = g.Acc(wanim->second.output);
                    zr_morph_track tr; std::memset(&tr, 0, sizeof(tr));
                    tr.num_targets = T; tr.first_key = (uint32_t)sc.morphTimes.size(); tr.num_keys = (uint32_t)in.count; tr.first_value = (uint32_t)sc.morphValues.size();
                    tr.first_rest = (uint32_t)sc.morphRestWeights.size(); tr.loop = 1; tr.t0 = 0.0f;
                    for (size_t k = 0; k < in.count; k++) sc.morphTimes.push_back(Gltf::Comp(in, k, 0));
                    for (size_t k = 0; k < in.count * T; k++) sc.morphValues.push_back(Gltf::Comp(out, k, 0));
                    sc.morphRestWeights.insert(sc.morphRestWeights.end(), nodeWeights.begin(), nodeWeights.end());
                    track = (int)sc.morphTracks.size();
                    sc.morphTracks.push_back(tr);
                }
            }
            if (mesh >= 0)
            {
                const size_t np = g.root.At("meshes").arr.at(mesh).At("primitives").Size();
                for (size_t pi = 0; pi < np; pi++)
                {
                    const MeshPrim& mp = prims.at({mesh, (int)pi});
                    zr_mesh_instance I; std::memset(&I, 0, sizeof(I));
                    float M[12]; ToToWorld(world, M);
                    I.base_vtx_offset = mp.vtx; I.base_idx_offset = mp.idx; I.mat_idx = (uint16_t)(mp.mat + 1);
                    if (skin >= 0)
                    {
                        I.base_vtx_offset = SkinPrimitive(nidx, skin, g.root.At("meshes").arr.at(mesh).At("primitives").arr.at(pi), mp);
                        Mat43 id; std::memset(&id, 0, sizeof(id)); for (int i = 0; i < 3; i++) id.m[i][i] = 1.0f;
                        ToToWorld(id, M);
                    }
                    if (morphed)
                    {   // a range of the node's own (the skin's copy, where the node is skinned too: one range listed in both tables)
                        if (skin < 0) I.base_vtx_offset = CopyPrimitive(mp);
                        MorphPrimitive(nidx, mesh, (int)pi, g.root.At("meshes").arr.at(mesh).At("primitives").arr.at(pi), mp, I.base_vtx_offset, track, nodeWeights);
                    }
                    FillMeshInstance(M, I);
                    const zr_material& mat = sc.materials.at((size_t)mp.mat + 1);
                    const uint32_t bct = mat.base_color_tex_subsurf_coat_weight & 0xffffu;
                    I.base_color_tex = (uint16_t)bct;
                    const float alpha = (float)((mat.base_color_factor >> 24) & 0xffu) / 255.0f, cutoff = (float)((mat.emissive_tex_alpha_cutoff_coat_ior >> 16) & 0xffu) / 255.0f;
                    I.alpha_factor_cutoff = (uint16_t)(Unorm8(alpha) | (Unorm8(cutoff) << 8));
                    I.base_emissive_tri_offset = 0xffffffffu;
                    const bool em = isEm(mp.mat);
                    const int alphaMode = (int)((mat.coat_color_flags >> 27) & 3u);
                    sc.instances.push_back(I);
                    if (entry != ZR_ANIM_ROOT && skin < 0) { sc.animInstIdx.push_back((uint32_t)sc.instances.size() - 1); sc.animInstNode.push_back(entry); }
                    sc.toWorld.insert(sc.toWorld.end(), M, M + 12);
                    sc.mask.push_back((uint8_t)((em ? ZR_SUBGROUP_EMISSIVE : ZR_SUBGROUP_NON_EMISSIVE) | (alphaMode != 0 ? ZR_INSTANCE_NON_OPAQUE : 0u)));
                    sc.numTris.push_back(mp.nidx / 3);
                    if (em) emissive.push_back(Em{(uint32_t)sc.instances.size() - 1, mp});
                }
            }
            if (const Json* ch = node.Find("children")) for (const Json& c : ch->arr) Visit((int)c.num, world, entry);
        }
    } walker{g, sc, prims, emissive, nodes, isEmissive, {}, nodeAnims, leadsToMesh, skins, leadsToJoint, isJoint, nodeEntry, skinnedPrims, meshTargets, meshWeights, weightAnims, {}};
    const Json& scenes = g.root.At("scenes");
    const Json& scene = scenes.arr.at((size_t)g.root.IntOr("scene", 0));
    for (const Json& n : scene.At("nodes").arr) walker.Visit((int)n.num, identity);
    if (!sc.animNodes.empty())
    {   // (an animated node outside the scene's node lists adds nothing.)  The tables are held to what zrh_scene_data_set_animation checks
        zr_anim_desc d; std::memset(&d, 0, sizeof(d));
        d.nodes = sc.animNodes.data(); d.num_nodes = (uint32_t)sc.animNodes.size(); d.keys = sc.animKeys.data(); d.num_keys = (uint32_t)sc.animKeys.size();
        d.instance_idx = sc.animInstIdx.data(); d.instance_node = sc.animInstNode.data(); d.num_instances = (uint32_t)sc.animInstIdx.size();
        char msg[256];
        if (ValidateAnimation(d, (uint32_t)sc.instances.size(), nullptr, msg, sizeof(msg))) Throw(std::string("glTF: animations: ") + msg);
        sc.anim = d; sc.hasAnim = true;
    }
    if (!skinnedPrims.empty())
    {   // the joint tables of the skins in use, one after the other; an influence's joint index counts from its skin's first joint
        if (nodeAnims.empty() && weightAnims.empty()) Throw("glTF: the file has a skin but no animation: nothing would pose it (skins are driven by zr_scene_animate)");
        for (size_t si = 0; si < skins.size(); si++)
        {
            SkinUse& u = skins[si];
            bool inUse = false; for (const SkinnedPrim& p : skinnedPrims) inUse = inUse || p.skin == (int)si;
            if (!inUse) continue;
            u.base = (uint32_t)sc.skinJoints.size();
            for (size_t j = 0; j < u.joints.size(); j++)
            {
                zr_skin_joint sj; sj.node = nodeEntry[(size_t)u.joints[j]];
                if (sj.node == ZR_ANIM_ROOT) Throw(u.name + "joint " + std::to_string(j) + " (node " + std::to_string(u.joints[j]) + ") is not part of the scene's node hierarchy");
                std::memcpy(sj.inverse_bind, u.ibm.data() + 12 * j, sizeof(sj.inverse_bind));
                sc.skinJoints.push_back(sj);
            }
        }
        if (sc.skinJoints.size() > 65535) Throw("glTF: skins: more than 65 535 joints in use");
        for (const SkinnedPrim& p : skinnedPrims)
        {
            const zr_skin_range& r = sc.skinRanges[p.range];
            for (uint32_t v = 0; v < r.num_vertices; v++) for (int k = 0; k < 4; k++) sc.skinInfluences[r.first_influence + v].joint[k] = (uint16_t)(sc.skinInfluences[r.first_influence + v].joint[k] + skins[(size_t)p.skin].base);
        }
        zr_skin_desc d; std::memset(&d, 0, sizeof(d));
        d.joints = sc.skinJoints.data(); d.num_joints = (uint32_t)sc.skinJoints.size(); d.ranges = sc.skinRanges.data(); d.num_ranges = (uint32_t)sc.skinRanges.size();
        d.influences = sc.skinInfluences.data(); d.num_influences = (uint32_t)sc.skinInfluences.size();
        char msg[256];
        if (zrsk::ValidateSkin(d, (uint32_t)sc.animNodes.size(), (uint32_t)sc.vertices.size(), msg, sizeof(msg))) Throw(std::string("glTF: skins: ") + msg);
        sc.skin = d; sc.hasSkin = true;
    }
    if (!sc.morphRanges.empty())
    {   // the tables are held to what zr_scene_set_morph checks
        sc.PointMorph();
        char msg[256];
        if (zrmo::ValidateMorph(sc.morph, sc.hasSkin ? &sc.skin : nullptr, (uint32_t)sc.vertices.size(), msg, sizeof(msg))) Throw(std::string("glTF: morph targets: ") + msg);
        sc.hasMorph = true;
    }
    else { sc.morphTracks.clear(); sc.morphTimes.clear(); sc.morphValues.clear(); sc.morphRestWeights.clear(); }
    // ---- emissive triangles in world space (glTF.cpp:692-767, SceneCore.cpp:196-236): ID = PCG3d(instance, 0, triangle).x
    for (const Em& em : emissive)
    {
        sc.instances[em.inst].base_emissive_tri_offset = (uint32_t)sc.emissives.size();
        const zr_material& mat = sc.materials.at((size_t)em.mp.mat + 1);
        const float* M = sc.toWorld.data() + 12 * (size_t)em.inst;
        for (uint32_t p = 0; p < em.mp.nidx / 3; p++)
        {
            float po[3][3], uv[6];
            for (int k = 0; k < 3; k++)
            {
                // (the instance's own vertices: the mesh's, or the copy a skinned / morphed node poses -- equal at rest, default morph weights applied)
                const zr_vertex& v = sc.vertices[sc.instances[em.inst].base_vtx_offset + sc.indices[em.mp.idx + 3 * p + k]];
                for (int r = 0; r < 3; r++) po[k][r] = v.pos[r];
                uv[2 * k] = v.uv[0]; uv[2 * k + 1] = v.uv[1];
            }
            uint32_t hx = em.inst, hy = 0, hz = p; zr_pcg3d(&hx, &hy, &hz);
            // the reference packs the triangle in OBJECT space when it loads the mesh (glTF.cpp:692-767) and SceneCore then decodes, transforms and
            // re-encodes it unless the instance's world matrix is the identity (SceneCore.cpp:196-236); the object-space record is kept for
            // zrh_emissive_to_world when the instance moves (UpdateEmissivePositions)
            zr_emissive_triangle e;
            PackEmissiveTriangle(po[0], po[1], po[2], uv, mat.emissive_factor_normal_scale & 0xffffffu, mat.emissive_tex_alpha_cutoff_coat_ior & 0xffffu,
                (uint16_t)(mat.emissive_strength_ior & 0xffffu), hx, (mat.coat_color_flags & (1u << ZR_MAT_DOUBLE_SIDED_BIT)) != 0, e);
            sc.emissivesInitial.push_back(e);
            static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            if (std::memcmp(M, kIdentity, sizeof(kIdentity)) != 0) { zr_emissive_triangle w; EmissiveToWorld(e, M, w); e = w; }
            sc.emissives.push_back(e);
        }
    }
}

} // namespace

extern "C" {

const char* zrh_scene_io_last_error(void) { return g_err.c_str(); }

int zrh_gltf_load(const char* path, const uint16_t* rho, const uint32_t* rhoDim, zrh_scene_data** out) { return zrh_gltf_load_ex(path, rho, rhoDim, 0u, out); }
// (a scene without textures has no blocks in either mode: its desc is the default mode's, and zr_scene_create takes it)
const zr_texture_blocks* zrh_scene_data_texture_blocks(const zrh_scene_data* s) { return s && s->keepCompressed && !s->texSources.empty() ? &s->blocks : nullptr; }
int zrh_gltf_load_ex(const char* path, const uint16_t* rho, const uint32_t* rhoDim, uint32_t flags, zrh_scene_data** out)
{
    if (!path || !out) { g_err = "null argument"; return -1; }
    if (flags & ~(uint32_t)(ZRH_LOAD_KEEP_COMPRESSED | ZRH_LOAD_JPEG | ZRH_LOAD_DEFORMED_LIGHTS)) { g_err = "zrh_gltf_load_ex: unknown flag"; return -1; }
    std::unique_ptr<zrh_scene_data> sc(new zrh_scene_data());
    sc->keepCompressed = (flags & ZRH_LOAD_KEEP_COMPRESSED) != 0; sc->loadJpeg = (flags & ZRH_LOAD_JPEG) != 0;
    sc->deformedLights = (flags & ZRH_LOAD_DEFORMED_LIGHTS) != 0;
    try { Load(path, *sc); }
    catch (const Error& e) { g_err = e.what; return -1; }
    catch (const std::exception& e) { g_err = std::string("glTF: malformed file (") + e.what() + ")"; return -1; }
    if (rho && rhoDim) { const size_t n = (size_t)rhoDim[0] * rhoDim[1] * rhoDim[2]; sc->rho.assign(rho, rho + n); for (int k = 0; k < 3; k++) sc->rhoDim[k] = rhoDim[k]; }
    sc->Finish();
    *out = sc.release();
    return 0;
}
const zr_scene_desc* zrh_scene_data_desc(const zrh_scene_data* s) { return s ? &s->desc : nullptr; }
void zrh_scene_data_tex_offsets(const zrh_scene_data* s, uint32_t* out4) { for (int k = 0; k < 4; k++) out4[k] = s->texOffsets[k]; }
void zrh_scene_data_destroy(zrh_scene_data* s) { delete s; }

void zrh_decompose_srt(const float* M, float* s, float* q, float* t) { DecomposeSRT(FromToWorld(M), s, q, t); }
int zrh_skin_pose(const zr_anim_desc* anim, const zr_skin_desc* skin, float t, const zr_vertex* rest, zr_vertex* out)
{
    if (!anim || !skin || ((!rest || !out) && skin->num_ranges)) { g_err = "zrh_skin_pose: null argument"; return -1; }
    uint64_t verts = 0;
    for (uint32_t r = 0; r < skin->num_ranges; r++) verts = std::max<uint64_t>(verts, (uint64_t)skin->ranges[r].first_vertex + skin->ranges[r].num_vertices);
    char msg[256];
    if (verts > 0xffffffffull || zrsk::ValidateSkin(*skin, anim->num_nodes, (uint32_t)verts, msg, sizeof(msg))) { g_err = std::string("zrh_skin_pose: ") + (verts > 0xffffffffull ? "a range wraps" : msg); return -1; }
    std::vector<float> world(12 * (size_t)anim->num_nodes), J(12 * (size_t)skin->num_joints);
    EvalNodeWorlds(*anim, t, world.data());
    zrsk::EvalJointMatrices(*skin, world.data(), J.data());
    zrsk::SkinRanges(*skin, J.data(), rest, out);
    return 0;
}
int zrh_morph_pose(const zr_anim_desc* anim, const zr_skin_desc* skin, const zr_morph_desc* morph, float t, const zr_vertex* rest, zr_vertex* out)
{
    if (!morph || (skin && !anim) || ((!rest || !out) && morph->num_ranges)) { g_err = "zrh_morph_pose: null argument"; return -1; }
    uint64_t verts = 0;
    for (uint32_t r = 0; r < morph->num_ranges && morph->ranges; r++) verts = std::max<uint64_t>(verts, (uint64_t)morph->ranges[r].first_vertex + morph->ranges[r].num_vertices);
    for (uint32_t r = 0; skin && r < skin->num_ranges && skin->ranges; r++) verts = std::max<uint64_t>(verts, (uint64_t)skin->ranges[r].first_vertex + skin->ranges[r].num_vertices);
    char msg[256];
    if (verts > 0xffffffffull) { g_err = "zrh_morph_pose: a range wraps"; return -1; }
    if (skin && zrsk::ValidateSkin(*skin, anim->num_nodes, (uint32_t)verts, msg, sizeof(msg))) { g_err = std::string("zrh_morph_pose: the skin: ") + msg; return -1; }
    if (zrmo::ValidateMorph(*morph, skin, (uint32_t)verts, msg, sizeof(msg))) { g_err = std::string("zrh_morph_pose: ") + msg; return -1; }
    std::vector<uint32_t> offs(morph->num_tracks);
    std::vector<float> W(zrmo::WeightOffsets(*morph, offs.data())), world, J;
    zrmo::EvalWeights(*morph, t, W.data());
    if (skin)
    {
        world.resize(12 * (size_t)anim->num_nodes); J.resize(12 * (size_t)skin->num_joints);
        EvalNodeWorlds(*anim, t, world.data());
        zrsk::EvalJointMatrices(*skin, world.data(), J.data());
    }
    zrmo::MorphRanges(*morph, W.data(), skin, J.data(), rest, out);
    return 0;
}
void zrh_compose_world(const float* s, const float* q, const float* t, const float* parent, float* out)
{
    Mat43 P; std::memset(&P, 0, sizeof(P)); for (int i = 0; i < 3; i++) P.m[i][i] = 1.0f;
    if (parent) P = FromToWorld(parent);
    ToToWorld(Mul(AffineTransformation(s, q, t), P), out);
}
void zrh_fill_mesh_instance(const float* M, zr_mesh_instance* inst) { FillMeshInstance(M, *inst); }
// ---- per-frame scene maintenance: what SceneCore::Update / TLAS::FillMeshInstanceData do for dynamic instances
void zrh_scene_data_begin_frame(zrh_scene_data* s)
{
    if (!s) return;
    s->prevWorld = s->toWorld;
    for (zr_mesh_instance& I : s->instances) InstanceBeginFrame(I);      // an instance that does not move this frame: Prev* = current, dTranslation = 0
    s->dirtyFirst = 0xffffffffu; s->dirtyEnd = 0;
    for (uint32_t i : s->movedIdx) s->movedSlot[i] = 0xffffffffu;
    s->movedIdx.clear(); s->movedWorld.clear();
}
int zrh_scene_data_set_instance_world(zrh_scene_data* s, uint32_t inst, const float* world)
{
    if (!s || !world || inst >= s->instances.size()) { g_err = "zrh_scene_data_set_instance_world: bad argument"; return -1; }
    if (s->prevWorld.size() != s->toWorld.size()) s->prevWorld = s->toWorld;
    zr_mesh_instance& I = s->instances[inst];
    // TLAS::FillMeshInstanceData, !staticMesh branch: current and previous S / R / T by decomposeSRT of the two world matrices
    InstanceSetWorld(I, world, s->prevWorld.data() + 12 * (size_t)inst);
    std::memcpy(s->toWorld.data() + 12 * (size_t)inst, world, 12 * sizeof(float));
    if (s->movedSlot.size() != s->instances.size()) s->movedSlot.assign(s->instances.size(), 0xffffffffu);
    if (s->movedSlot[inst] == 0xffffffffu) { s->movedSlot[inst] = (uint32_t)s->movedIdx.size(); s->movedIdx.push_back(inst); s->movedWorld.resize(12 * s->movedIdx.size()); }
    std::memcpy(s->movedWorld.data() + 12 * (size_t)s->movedSlot[inst], world, 12 * sizeof(float));
    // SceneCore::UpdateEmissivePositions for an instance that carries lights
    if (I.base_emissive_tri_offset != 0xffffffffu && !s->emissivesInitial.empty())
    {
        const uint32_t b = I.base_emissive_tri_offset, n = s->numTris[inst];
        for (uint32_t k = b; k < b + n; k++) EmissiveToWorld(s->emissivesInitial[k], world, s->emissives[k]);
        s->dirtyFirst = std::min(s->dirtyFirst, b); s->dirtyEnd = std::max(s->dirtyEnd, b + n);
    }
    return 0;
}
void zrh_scene_data_dirty_emissives(const zrh_scene_data* s, uint32_t* first, uint32_t* count)
{
    const bool any = s && s->dirtyEnd > s->dirtyFirst;
    *first = any ? s->dirtyFirst : 0u; *count = any ? s->dirtyEnd - s->dirtyFirst : 0u;
}
uint32_t zrh_scene_data_moved(const zrh_scene_data* s, const uint32_t** idx, const float** world)
{
    if (!s) return 0;
    if (idx) *idx = s->movedIdx.data();
    if (world) *world = s->movedWorld.data();
    return (uint32_t)s->movedIdx.size();
}
// ---- keyframe animation: the host path (include/zr_anim.h on the host, then set_instance_world in list order)
static void ClearMorph(zrh_scene_data* s);
int zrh_scene_data_set_animation(zrh_scene_data* s, const zr_anim_desc* d)
{
    if (!s) { g_err = "zrh_scene_data_set_animation: null scene"; return -1; }
    if (!d || (!d->num_nodes && !d->num_instances))
    { zrh_scene_data_set_skinning(s, nullptr); s->hasAnim = false; s->animNodes.clear(); s->animKeys.clear(); s->animInstIdx.clear(); s->animInstNode.clear(); std::memset(&s->anim, 0, sizeof(s->anim)); return 0; }
    char msg[256];
    if (ValidateAnimation(*d, (uint32_t)s->instances.size(), nullptr, msg, sizeof(msg))) { g_err = std::string("zrh_scene_data_set_animation: ") + msg; return -1; }
    zrh_scene_data_set_skinning(s, nullptr);      // a skin belongs to the animation it was set on (zr_scene_set_animation does the same); the morph set goes with it
    s->animNodes.assign(d->nodes, d->nodes + d->num_nodes); s->animKeys.assign(d->keys, d->keys + d->num_keys);
    s->animInstIdx.assign(d->instance_idx, d->instance_idx + d->num_instances); s->animInstNode.assign(d->instance_node, d->instance_node + d->num_instances);
    s->anim.nodes = s->animNodes.data(); s->anim.num_nodes = d->num_nodes; s->anim.keys = s->animKeys.data(); s->anim.num_keys = d->num_keys;
    s->anim.instance_idx = s->animInstIdx.data(); s->anim.instance_node = s->animInstNode.data(); s->anim.num_instances = d->num_instances;
    s->hasAnim = true;
    return 0;
}
const zr_anim_desc* zrh_scene_data_animation(const zrh_scene_data* s) { return s && s->hasAnim ? &s->anim : nullptr; }
const zr_skin_desc* zrh_scene_data_skinning(const zrh_scene_data* s) { return s && s->hasSkin ? &s->skin : nullptr; }
int zrh_scene_data_set_skinning(zrh_scene_data* s, const zr_skin_desc* d)
{
    if (!s) { g_err = "zrh_scene_data_set_skinning: null scene"; return -1; }
    if (!d || (!d->num_joints && !d->num_ranges && !d->num_influences))
    { ClearMorph(s); s->hasSkin = false; s->skinJoints.clear(); s->skinRanges.clear(); s->skinInfluences.clear(); std::memset(&s->skin, 0, sizeof(s->skin)); return 0; }
    if (!s->hasAnim) { g_err = "zrh_scene_data_set_skinning: no animation set (zrh_scene_data_set_animation): the joints are nodes of its table"; return -1; }
    char msg[256];
    if (zrsk::ValidateSkin(*d, s->anim.num_nodes, (uint32_t)s->vertices.size(), msg, sizeof(msg))) { g_err = std::string("zrh_scene_data_set_skinning: ") + msg; return -1; }
    ClearMorph(s);      // a morph set is laid out against the skin set it was set after (zr_scene_set_skinning does the same)
    s->skinJoints.assign(d->joints, d->joints + d->num_joints); s->skinRanges.assign(d->ranges, d->ranges + d->num_ranges);
    s->skinInfluences.assign(d->influences, d->influences + d->num_influences);
    s->skin.joints = s->skinJoints.data(); s->skin.num_joints = d->num_joints; s->skin.ranges = s->skinRanges.data(); s->skin.num_ranges = d->num_ranges;
    s->skin.influences = s->skinInfluences.data(); s->skin.num_influences = d->num_influences;
    s->hasSkin = true;
    return 0;
}
const zr_vertex* zrh_scene_data_skin_pose(zrh_scene_data* s, float t)
{
    if (!s || !s->hasSkin || !s->hasAnim) { g_err = "zrh_scene_data_skin_pose: no skin set"; return nullptr; }
    s->skinRest.clear();
    for (const zr_skin_range& r : s->skinRanges) s->skinRest.insert(s->skinRest.end(), s->vertices.begin() + r.first_vertex, s->vertices.begin() + r.first_vertex + r.num_vertices);
    s->skinPosed.resize(s->skinRest.size() + 1);      // (+ 1: a pointer that is not null for a set without vertices)
    if (zrh_skin_pose(&s->anim, &s->skin, t, s->skinRest.data(), s->skinPosed.data())) return nullptr;
    return s->skinPosed.data();
}
const zr_morph_desc* zrh_scene_data_morph(const zrh_scene_data* s) { return s && s->hasMorph ? &s->morph : nullptr; }
static void ClearMorph(zrh_scene_data* s)
{
    s->hasMorph = false; s->morphTracks.clear(); s->morphTargets.clear(); s->morphRanges.clear(); s->morphTimes.clear(); s->morphValues.clear();
    s->morphRestWeights.clear(); s->morphDeltas.clear(); std::memset(&s->morph, 0, sizeof(s->morph));
}
int zrh_scene_data_set_morph(zrh_scene_data* s, const zr_morph_desc* d)
{
    if (!s) { g_err = "zrh_scene_data_set_morph: null scene"; return -1; }
    if (!d || (!d->num_tracks && !d->num_targets && !d->num_ranges)) { ClearMorph(s); return 0; }
    if (!s->hasAnim) { g_err = "zrh_scene_data_set_morph: no animation set (zrh_scene_data_set_animation)"; return -1; }
    char msg[256];
    if (zrmo::ValidateMorph(*d, s->hasSkin ? &s->skin : nullptr, (uint32_t)s->vertices.size(), msg, sizeof(msg))) { g_err = std::string("zrh_scene_data_set_morph: ") + msg; return -1; }
    const zr_morph_desc c = *d;      // (d may point into this scene's own vectors)
    std::vector<zr_morph_track> tracks(c.tracks, c.tracks + c.num_tracks); std::vector<zr_morph_target> targets(c.targets, c.targets + c.num_targets);
    std::vector<zr_morph_range> ranges(c.ranges, c.ranges + c.num_ranges); std::vector<float> times(c.times, c.times + c.num_times), values(c.values, c.values + c.num_values),
        rest(c.rest_weights, c.rest_weights + c.num_rest_weights), deltas(c.deltas, c.deltas + 3 * (size_t)c.num_deltas);
    s->morphTracks.swap(tracks); s->morphTargets.swap(targets); s->morphRanges.swap(ranges); s->morphTimes.swap(times); s->morphValues.swap(values);
    s->morphRestWeights.swap(rest); s->morphDeltas.swap(deltas);
    s->PointMorph();
    s->hasMorph = true;
    return 0;
}
const zr_vertex* zrh_scene_data_morph_pose(zrh_scene_data* s, float t)
{
    if (!s || !s->hasMorph || !s->hasAnim) { g_err = "zrh_scene_data_morph_pose: no morph set"; return nullptr; }
    s->morphRest.clear();
    for (const zr_morph_range& r : s->morphRanges) s->morphRest.insert(s->morphRest.end(), s->vertices.begin() + r.first_vertex, s->vertices.begin() + r.first_vertex + r.num_vertices);
    s->morphPosed.resize(s->morphRest.size() + 1);      // (+ 1: a pointer that is not null for a set without vertices)
    if (zrh_morph_pose(&s->anim, s->hasSkin ? &s->skin : nullptr, &s->morph, t, s->morphRest.data(), s->morphPosed.data())) return nullptr;
    return s->morphPosed.data();
}
void zrh_scene_data_set_device_morph(zrh_scene_data* s, int on) { if (s) s->deviceMorph = on != 0; }
int zrh_scene_data_device_morph(const zrh_scene_data* s) { return s && s->deviceMorph ? 1 : 0; }
void zrh_scene_data_set_device_skinning(zrh_scene_data* s, int on) { if (s) s->deviceSkinning = on != 0; }
int zrh_scene_data_device_skinning(const zrh_scene_data* s) { return s && s->deviceSkinning ? 1 : 0; }
int zrh_scene_data_animate(zrh_scene_data* s, float t)
{
    if (!s || !s->hasAnim) { g_err = "zrh_scene_data_animate: no animation set"; return -1; }
    s->animWorld.resize(12 * (size_t)s->anim.num_nodes);
    EvalNodeWorlds(s->anim, t, s->animWorld.data());
    for (uint32_t j = 0; j < s->anim.num_instances; j++)
        if (zrh_scene_data_set_instance_world(s, s->animInstIdx[j], s->animWorld.data() + 12 * (size_t)s->animInstNode[j])) return -1;
    return 0;
}
void zrh_scene_data_set_device_animation(zrh_scene_data* s, int on) { if (s) s->deviceAnimation = on != 0; }
int zrh_scene_data_device_animation(const zrh_scene_data* s) { return s && s->deviceAnimation ? 1 : 0; }
void zrh_scene_data_set_device_records(zrh_scene_data* s, int on) { if (s) s->deviceRecords = on != 0; }
int zrh_scene_data_device_records(const zrh_scene_data* s) { return s && s->deviceRecords ? 1 : 0; }
int zrh_scene_data_from_desc(const zr_scene_desc* d, const zr_emissive_triangle* object_space_emissives, zrh_scene_data** out)
{
    if (!d || !out || !d->vertices || !d->indices || !d->instances || !d->instance_to_world || !d->instance_mask || !d->instance_num_tris || !d->materials || !d->rho_lut ||
        (d->num_emissives && !d->emissives))
    { g_err = "zrh_scene_data_from_desc: incomplete scene description"; return -1; }
    std::unique_ptr<zrh_scene_data> sc(new zrh_scene_data());
    sc->vertices.assign(d->vertices, d->vertices + d->num_vertices); sc->indices.assign(d->indices, d->indices + d->num_indices);
    sc->instances.assign(d->instances, d->instances + d->num_instances); sc->toWorld.assign(d->instance_to_world, d->instance_to_world + 12 * (size_t)d->num_instances);
    sc->mask.assign(d->instance_mask, d->instance_mask + d->num_instances); sc->numTris.assign(d->instance_num_tris, d->instance_num_tris + d->num_instances);
    sc->materials.assign(d->materials, d->materials + d->num_materials);
    if (d->num_emissives) sc->emissives.assign(d->emissives, d->emissives + d->num_emissives);
    if (d->num_emissives && object_space_emissives) sc->emissivesInitial.assign(object_space_emissives, object_space_emissives + d->num_emissives);
    sc->rho.assign(d->rho_lut, d->rho_lut + (size_t)d->rho_dim[0] * d->rho_dim[1] * d->rho_dim[2]); for (int k = 0; k < 3; k++) sc->rhoDim[k] = d->rho_dim[k];
    if (d->num_textures && d->textures) sc->textures.assign(d->textures, d->textures + d->num_textures);
    if (d->texel_bytes && d->texels) sc->texels.assign(d->texels, d->texels + d->texel_bytes);
    sc->Finish();
    *out = sc.release();
    return 0;
}
void zrh_emissive_to_world(const zr_emissive_triangle* in, const float* to_world_3x4, zr_emissive_triangle* out) { zr_emissive_triangle t; EmissiveToWorld(*in, to_world_3x4, t); *out = t; }
void zrh_emissive_from_vertices(const zr_emissive_triangle* rec, const float* p0, const float* p1, const float* p2, const float* to_world_3x4,
    zr_emissive_triangle* object_out, zr_emissive_triangle* world_out)
{ zr_emissive_triangle o, w; EmissiveFromVertices(*rec, p0, p1, p2, to_world_3x4, o, w); *object_out = o; *world_out = w; }
// the light triangles of instance i are [base_emissive_tri_offset, + numTris): triangle k's owner, or instances.size() for none
static size_t LightOwner(const zrh_scene_data* s, uint32_t k)
{
    for (size_t i = 0; i < s->instances.size(); i++)
    {
        const uint32_t b = s->instances[i].base_emissive_tri_offset;
        if (b != 0xffffffffu && k >= b && k - b < s->numTris[i]) return i;
    }
    return s->instances.size();
}
int zrh_scene_data_refresh_emissives(zrh_scene_data* s, const zr_vertex* vertices, uint32_t first_tri, uint32_t count)
{
    if (!s) { g_err = "zrh_scene_data_refresh_emissives: null scene"; return -1; }
    if ((uint64_t)first_tri + count > s->emissives.size()) { g_err = "zrh_scene_data_refresh_emissives: the range exceeds the scene's emissive triangles"; return -1; }
    if (!s->emissives.empty() && s->emissivesInitial.empty()) { g_err = "zrh_scene_data_refresh_emissives: the scene has no object-space light records"; return -1; }
    const zr_vertex* V = vertices ? vertices : s->vertices.data();
    size_t owner = s->instances.size();
    for (uint32_t k = first_tri; k < first_tri + count; k++)
    {
        // (triangles of one instance follow each other: the owner is looked up when the range leaves it)
        if (owner == s->instances.size() || k < s->instances[owner].base_emissive_tri_offset || k - s->instances[owner].base_emissive_tri_offset >= s->numTris[owner]) owner = LightOwner(s, k);
        if (owner == s->instances.size()) continue;
        const zr_mesh_instance& I = s->instances[owner];
        const uint64_t at = (uint64_t)I.base_idx_offset + 3ull * (k - I.base_emissive_tri_offset);
        if (at + 3 > s->indices.size()) continue;
        const uint64_t v[3] = {(uint64_t)I.base_vtx_offset + s->indices[at], (uint64_t)I.base_vtx_offset + s->indices[at + 1], (uint64_t)I.base_vtx_offset + s->indices[at + 2]};
        if (v[0] >= s->vertices.size() || v[1] >= s->vertices.size() || v[2] >= s->vertices.size()) continue;
        zr_emissive_triangle o, w;
        EmissiveFromVertices(s->emissivesInitial[k], V[v[0]].pos, V[v[1]].pos, V[v[2]].pos, s->toWorld.data() + 12 * owner, o, w);
        s->emissivesInitial[k] = o; s->emissives[k] = w;
        s->dirtyFirst = std::min(s->dirtyFirst, k); s->dirtyEnd = std::max(s->dirtyEnd, k + 1);
    }
    return 0;
}
uint32_t zrh_scene_data_pose_lights(zrh_scene_data* s, const uint32_t** tris)
{
    if (tris) *tris = nullptr;
    if (!s) return 0;
    s->poseLights.clear();
    auto posed = [s](uint64_t v)
    {
        if (s->hasSkin) for (const zr_skin_range& r : s->skinRanges) if (v >= r.first_vertex && v - r.first_vertex < r.num_vertices) return true;
        if (s->hasMorph) for (const zr_morph_range& r : s->morphRanges) if (v >= r.first_vertex && v - r.first_vertex < r.num_vertices) return true;
        return false;
    };
    if ((s->hasSkin || s->hasMorph) && !s->emissives.empty())
        for (size_t i = 0; i < s->instances.size(); i++)
        {
            const zr_mesh_instance& I = s->instances[i];
            if (I.base_emissive_tri_offset == 0xffffffffu) continue;
            for (uint32_t t = 0; t < s->numTris[i]; t++)
            {
                const uint64_t at = (uint64_t)I.base_idx_offset + 3ull * t, k = (uint64_t)I.base_emissive_tri_offset + t;
                if (at + 3 > s->indices.size() || k >= s->emissives.size()) break;
                if (posed((uint64_t)I.base_vtx_offset + s->indices[at]) || posed((uint64_t)I.base_vtx_offset + s->indices[at + 1]) || posed((uint64_t)I.base_vtx_offset + s->indices[at + 2]))
                    s->poseLights.push_back((uint32_t)k);
            }
        }
    std::sort(s->poseLights.begin(), s->poseLights.end());
    if (tris) *tris = s->poseLights.data();
    return (uint32_t)s->poseLights.size();
}
const zr_emissive_triangle* zrh_scene_data_initial_emissives(const zrh_scene_data* s) { return s && !s->emissivesInitial.empty() ? s->emissivesInitial.data() : nullptr; }
void zrh_pack_emissive_triangle(const float* v0, const float* v1, const float* v2, const float* uv6, uint32_t factor, uint32_t tex, uint16_t strength, uint32_t id,
    int doubleSided, zr_emissive_triangle* out) { PackEmissiveTriangle(v0, v1, v2, uv6, factor, tex, strength, id, doubleSided != 0, *out); }

int zrh_png_decode(const char* name, const uint8_t* data, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* rgba8, size_t capacity)
{
    if (!data || !w || !h) { g_err = "zrh_png_decode: null argument"; return -1; }
    try
    {
        const Png png = DecodePng(name ? name : "<memory>", data, bytes);
        *w = png.w; *h = png.h;
        if (rgba8)
        {
            if (capacity < png.rgba.size()) Throw(std::string(name ? name : "<memory>") + ": the output buffer is smaller than the image");
            std::memcpy(rgba8, png.rgba.data(), png.rgba.size());
        }
    }
    catch (const Error& e) { g_err = e.what; return -1; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    return 0;
}
int zrh_jpeg_decode(const char* name, const uint8_t* data, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* rgba8, size_t capacity)
{
    if (!data || !w || !h) { g_err = "zrh_jpeg_decode: null argument"; return -1; }
    try
    {
        const std::string nm = name ? name : "<memory>";
        const std::vector<uint8_t> rec = JpegRecord(PackJpeg(nm, data, bytes, zrjp::kMapRgba));
        zrjp::Header hd;
        if (!rgba8)
        {
            if (const char* why = zrjp::CheckRecord(rec.data(), rec.size(), &hd)) Throw(nm + ": invalid JPEG coefficient record: " + why);
            *w = hd.w; *h = hd.h;
            return 0;
        }
        const std::vector<uint8_t> px = ExpandJpegRecord(nm, rec.data(), rec.size(), hd);
        *w = hd.w; *h = hd.h;
        if (capacity < px.size()) Throw(nm + ": the output buffer is smaller than the image");
        std::memcpy(rgba8, px.data(), px.size());
    }
    catch (const Error& e) { g_err = e.what; return -1; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    return 0;
}
int zrh_jpeg_pack(const char* name, const uint8_t* data, size_t bytes, uint32_t channel_map, uint8_t* record, size_t capacity, size_t* record_bytes)
{
    if (!data || !record_bytes) { g_err = "zrh_jpeg_pack: null argument"; return -1; }
    if (channel_map > (uint32_t)zrjp::kMapBg) { g_err = "zrh_jpeg_pack: unknown channel map"; return -1; }
    try
    {
        const std::string nm = name ? name : "<memory>";
        const std::vector<uint8_t> rec = JpegRecord(PackJpeg(nm, data, bytes, channel_map));
        *record_bytes = rec.size();
        if (record)
        {
            if (capacity < rec.size()) Throw(nm + ": the output buffer is smaller than the record");
            std::memcpy(record, rec.data(), rec.size());
        }
    }
    catch (const Error& e) { g_err = e.what; return -1; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    return 0;
}
int zrh_jpeg_expand(const uint8_t* record, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* texels, size_t capacity)
{
    if (!record || !w || !h) { g_err = "zrh_jpeg_expand: null argument"; return -1; }
    try
    {
        zrjp::Header hd;
        if (!texels)
        {
            if (const char* why = zrjp::CheckRecord(record, bytes, &hd)) Throw(std::string("zrh_jpeg_expand: invalid JPEG coefficient record: ") + why);
            *w = hd.w; *h = hd.h;
            return 0;
        }
        const std::vector<uint8_t> px = ExpandJpegRecord("zrh_jpeg_expand", record, bytes, hd);
        *w = hd.w; *h = hd.h;
        if (capacity < px.size()) Throw("zrh_jpeg_expand: the output buffer is smaller than the image");
        std::memcpy(texels, px.data(), px.size());
    }
    catch (const Error& e) { g_err = e.what; return -1; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    return 0;
}
int zrh_mip_generate(const zr_texture_desc* descs, uint32_t n, uint8_t* texels)
{
    if (n && (!descs || !texels)) { g_err = "zrh_mip_generate: null argument"; return -1; }
    for (uint32_t i = 0; i < n; i++)
    {
        if (!descs[i].num_mips || !descs[i].width || !descs[i].height || descs[i].format > ZR_TEX_RG8) { g_err = "zrh_mip_generate: texture " + std::to_string(i) + " is malformed"; return -1; }
        zrmg::GenerateChain(&descs[i], texels);
    }
    return 0;
}
int zrh_bc7_decode(const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* rgba)
{
    const uint32_t bw = (w + 3) / 4, bh = (h + 3) / 4;
    for (uint32_t by = 0; by < bh; by++) for (uint32_t bx = 0; bx < bw; bx++)
    {
        uint8_t px[16][4];
        Bc7Block(blocks + 16 * ((size_t)by * bw + bx), px);
        for (int i = 0; i < 16; i++)
        {
            const uint32_t x = 4 * bx + (i & 3), y = 4 * by + (i >> 2);
            if (x < w && y < h) std::memcpy(rgba + 4 * ((size_t)y * w + x), px[i], 4);
        }
    }
    return 0;
}
int zrh_bc5_decode(const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* rg)
{
    const uint32_t bw = (w + 3) / 4, bh = (h + 3) / 4;
    for (uint32_t by = 0; by < bh; by++) for (uint32_t bx = 0; bx < bw; bx++)
    {
        uint8_t r[16], g[16];
        const uint8_t* b = blocks + 16 * ((size_t)by * bw + bx);
        Bc4Block(b, r); Bc4Block(b + 8, g);
        for (int i = 0; i < 16; i++)
        {
            const uint32_t x = 4 * bx + (i & 3), y = 4 * by + (i >> 2);
            if (x < w && y < h) { rg[2 * ((size_t)y * w + x)] = r[i]; rg[2 * ((size_t)y * w + x) + 1] = g[i]; }
        }
    }
    return 0;
}

}
