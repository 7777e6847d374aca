// TEST-ONLY, stand-alone: the loader's deformed-light path (ZRH_LOAD_DEFORMED_LIGHTS, zetaray_amd/host/zr_scene_io.cpp) and the host form of the light
// refresh (zrh_scene_data_pose_lights, zrh_scene_data_refresh_emissives) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.  Loads the emissive
// variants of the morph and the skin fixture (argv[1..]: tests/lightmath/cases.py lays them out) and damaged variants of each -- indices accessors, counts,
// offsets, views, materials and meshes out of range.  Every variant must be refused (-1 with a message) or load with light tables that hold: each listed
// light triangle's indices are followed, the sets are posed by the host form and every light triangle is refreshed from the posed vertices.  Prints the
// counts; exit status 1 when an intact fixture does not load with lights to pose, or a loaded variant's tables do not hold.  `make -C tests/lightmath fuzz`.
#include "../../zetaray_amd/host/zr_scene_io.h"
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

static std::vector<char> Read(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }
static void Write(const std::string& p, const char* d, size_t n) { std::ofstream f(p, std::ios::binary | std::ios::trunc); f.write(d, (std::streamsize)n); }

static int g_loaded = 0, g_refused = 0, g_bad = 0;
static const uint16_t kRho[1] = {0};
static const uint32_t kRhoDim[3] = {1, 1, 1};

// the light tables of a loaded scene: every index followed, the pose applied, every record re-derived.  *posedLights: how many lights the sets touch
static bool LightsHold(zrh_scene_data* s, uint32_t* posedLights)
{
    const zr_scene_desc* d = zrh_scene_data_desc(s);
    const zr_anim_desc* a = zrh_scene_data_animation(s);
    const zr_skin_desc* k = zrh_scene_data_skinning(s);
    const zr_morph_desc* m = zrh_scene_data_morph(s);
    volatile double sum = 0;
    for (uint32_t i = 0; i < d->num_instances; i++)
    {
        const zr_mesh_instance& I = d->instances[i];
        if (I.base_emissive_tri_offset == 0xffffffffu) continue;
        if ((uint64_t)I.base_emissive_tri_offset + d->instance_num_tris[i] > d->num_emissives) return false;
        if ((uint64_t)I.base_idx_offset + 3ull * d->instance_num_tris[i] > d->num_indices) return false;
        for (uint32_t t = 0; t < 3 * d->instance_num_tris[i]; t++) if ((uint64_t)I.base_vtx_offset + d->indices[I.base_idx_offset + t] >= d->num_vertices) return false;
    }
    const uint32_t* tris = nullptr;
    const uint32_t n = zrh_scene_data_pose_lights(s, &tris);
    *posedLights = n;
    for (uint32_t j = 0; j < n; j++) { if (tris[j] >= d->num_emissives || (j && tris[j] <= tris[j - 1])) return false; sum += d->emissives[tris[j]].vtx0[0]; }
    if (!d->num_emissives) return true;
    if (!zrh_scene_data_initial_emissives(s)) return a == nullptr;      // (object-space records come with an animation)
    // the posed vertex array, as zrh_scene_animate's host path makes it
    std::vector<zr_vertex> all(d->vertices, d->vertices + d->num_vertices);
    if (k && a)
    {
        const zr_vertex* posed = zrh_scene_data_skin_pose(s, 0.6f);
        if (!posed) return false;
        for (uint32_t r = 0; r < k->num_ranges; r++) { std::memcpy(all.data() + k->ranges[r].first_vertex, posed, (size_t)k->ranges[r].num_vertices * sizeof(zr_vertex)); posed += k->ranges[r].num_vertices; }
    }
    if (m && a)
    {
        const zr_vertex* posed = zrh_scene_data_morph_pose(s, 0.6f);
        if (!posed) return false;
        for (uint32_t r = 0; r < m->num_ranges; r++) { std::memcpy(all.data() + m->ranges[r].first_vertex, posed, (size_t)m->ranges[r].num_vertices * sizeof(zr_vertex)); posed += m->ranges[r].num_vertices; }
    }
    zrh_scene_data_begin_frame(s);
    if (zrh_scene_data_refresh_emissives(s, all.data(), 0, d->num_emissives)) return false;
    if (zrh_scene_data_refresh_emissives(s, nullptr, d->num_emissives / 2, d->num_emissives - d->num_emissives / 2)) return false;
    if (!zrh_scene_data_refresh_emissives(s, all.data(), 1, d->num_emissives)) return false;      // one past the end: refused
    uint32_t first = 0, count = 0;
    zrh_scene_data_dirty_emissives(s, &first, &count);
    if ((uint64_t)first + count > d->num_emissives) return false;
    for (uint32_t t = 0; t < d->num_emissives; t++) sum += d->emissives[t].vtx0[1] + zrh_scene_data_initial_emissives(s)[t].vtx0[2];
    return true;
}
static int Try(const std::string& gltf, uint32_t* posedLights)
{
    zrh_scene_data* s = nullptr;
    *posedLights = 0;
    if (zrh_gltf_load_ex(gltf.c_str(), kRho, kRhoDim, ZRH_LOAD_DEFORMED_LIGHTS, &s) != 0) { g_refused++; return -1; }
    if (!LightsHold(s, posedLights)) { g_bad++; std::fprintf(stderr, "light tables do not hold: %s\n", gltf.c_str()); }
    g_loaded++;
    zrh_scene_data_destroy(s);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: fuzz_lights FILE.gltf ... (the emissive fixtures laid out by tests/lightmath/cases.py)\n"); return 2; }
    int variants = 0;
    for (int f = 1; f < argc; f++)
    {
        const std::string gltf = argv[f], var = gltf.substr(0, gltf.rfind('/') + 1) + "variant.gltf";
        const std::vector<char> text = Read(gltf);
        if (text.empty()) { std::fprintf(stderr, "no fixture at %s\n", gltf.c_str()); return 2; }
        uint32_t lights = 0;
        if (Try(gltf, &lights) != 0 || g_bad || !lights) { std::fprintf(stderr, "%s: the intact fixture does not load with lights to pose (%u): %s\n", gltf.c_str(), lights, zrh_scene_io_last_error()); return 1; }
        // without the flag the same file is refused
        zrh_scene_data* s = nullptr;
        if (zrh_gltf_load_ex(gltf.c_str(), kRho, kRhoDim, 0u, &s) == 0) { std::fprintf(stderr, "%s: loaded without ZRH_LOAD_DEFORMED_LIGHTS\n", gltf.c_str()); return 1; }
        const std::string json(text.begin(), text.end());
        const char* keys[] = {"\"indices\":", "\"count\":", "\"byteOffset\":", "\"bufferView\":", "\"POSITION\":", "\"material\":", "\"mesh\":", "\"skin\":", "\"JOINTS_0\":"};
        const char* values[] = {"1", "99999", "4000000000"};
        for (const char* key : keys)
            for (size_t at = json.find(key); at != std::string::npos; at = json.find(key, at + 1))
            {
                size_t b = at + std::strlen(key); while (b < json.size() && json[b] == ' ') b++;
                size_t e = b; while (e < json.size() && (std::isdigit((unsigned char)json[e]) || json[e] == '-' || json[e] == '.')) e++;
                if (e == b) continue;
                for (const char* v : values)
                {
                    const std::string m = json.substr(0, b) + v + json.substr(e);
                    Write(var, m.data(), m.size()); Try(var, &lights); variants++;
                }
            }
    }
    std::printf("fuzz_lights: %d variants + %d intact fixtures: %d loaded with light tables that hold, %d refused, %d with tables that do not hold\n", variants, argc - 1, g_loaded, g_refused, g_bad);
    return g_bad ? 1 : 0;
}
