// FrequenSee.hpp — C++17 host-side mirror of the reference's plugin interface, over the C ABI only
// (include/frequensee.h; no HIP headers needed by the includer).
//
//   frequensee::AudioRayTracingSubsystem  <->  UAudioRayTracingSubsystem  (Public/AudioRayTracingSubsystem.h:86-196)
//   frequensee::FrequenSeeAudioComponent  <->  UFrequenSeeAudioComponent  (Public/FrequenSeeAudioComponent.h:20-154)
//   frequensee::MaterialAcousticProcessor <->  UMaterialAcousticProcessor (Public/MaterialAcousticProcessor.h:55-70)
//
// Same member names and argument meaning as the reference so a UE shim or a headless
// harness reads like the original call sites.  check()-style aborts of the reference become
// std::runtime_error carrying fs_last_error().
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/frequensee.h"

namespace frequensee {

struct FVector {
    float X = 0, Y = 0, Z = 0;
};

class AudioRayTracingSubsystem;
class MaterialAcousticProcessor;

// UAcousticGeometryComponent (Public/AcousticGeometryComponent.h:9-22) + the owner's collision triangles
struct AcousticGeometryComponent {
    std::vector<float> Triangles;     // [T][3][3], cm
    std::vector<uint16_t> MaterialId; // [T] index into the material table (UAcousticMaterial per actor)
    uint32_t Actor = 0;               // AActor the collision belongs to
};

class FrequenSeeAudioComponent {
public:
    explicit FrequenSeeAudioComponent(FVector Location = {}) : Location_(Location) {}
    FrequenSeeAudioComponent(const FrequenSeeAudioComponent&) = delete;
    FrequenSeeAudioComponent& operator=(const FrequenSeeAudioComponent&) = delete;
    ~FrequenSeeAudioComponent();

    void OnRegister(AudioRayTracingSubsystem& SubSys);   // FrequenSeeAudioComponent.cpp:42-52
    void OnUnregister();                                 // :54-64

    FVector GetComponentLocation() const { return Location_; }
    void SetComponentLocation(FVector L);
    // source directivity: the owner's GetForwardVector() before a trace, and per-band gains [bands][samples] over
    // 0 .. 180 degrees from it (empty: omnidirectional again) — fs_source_set_orientation / fs_source_set_directivity
    void SetForwardVector(FVector F);
    void SetDirectivity(const std::vector<float>& Gains, int Samples);
    // order window: traced frames keep only the paths with MinOrder .. MaxOrder nodes made by a hit (both included;
    // (0, FS_ORDER_UNBOUNDED): everything).  Direct renderer alone: MinOrder = 1; first-order voices too: 2; second-order too: 3
    // — fs_source_set_order_window / fs_source_get_order_window
    void SetOrderWindow(int MinOrder, int MaxOrder = FS_ORDER_UNBOUNDED);
    void GetOrderWindow(int& MinOrder, int& MaxOrder) const;

    int NumBins() const;      // FrequenSeeAudioComponent.h:137
    int NumSamples() const;   // :138

    void FlushEnergyBuffer();                                            // .h:76-79
    void UpdateEnergyBuffer(const std::vector<float>& NewEnergyValues);  // .h:81-85
    void AddEnergyAtDelay(float DelaySeconds, float EnergyValue, int Band = 0);   // .h:87-91
    std::vector<float> EnergyBuffer() const;                             // [bands][NumBins]
    void ReconstructImpulseResponse();                                   // .cpp:320-380
    // GetImpulseResponse()[Channel]: pointer into the published front buffer (lock-free, audio thread safe)
    const float* GetImpulseResponse(int Channel, int* NumSamplesOut = nullptr) const;   // .h:113
    float GetOcclusionAttenuation() const;                               // .h:112
    fs_sound_result UpdateSound(uint64_t Seed = 0x5EED);                 // .cpp:283-306
    void SaveImpulseResponse(const std::string& Path, int Channel = 0) const;   // SaveArrayToFile .cpp:492-505
    // GetImpulseResponse() is a mutable reference in the reference (.h:113): install an IR of the caller's own
    void SetImpulseResponse(const std::vector<float>& IR);
    // GenerateDummyImpulseResponse (.cpp:408-452) as it ends up: a delta at samples 0 and N-1
    std::vector<float> GenerateDummyImpulseResponse();
    // the room parameters published with the front IR by a reconstruct with FS_FLAG_ROOM_PARAMETERS (one record per band; empty and
    // *Sequence = 0 when that publish carries none) — fs_get_room_parameters, lock-free
    std::vector<fs_room_parameters> GetRoomParameters(uint64_t* Sequence = nullptr) const;
    // not in the reference (its occlusion plugin is a no-op): this source's direct sound — distance, arrival time, visibility and
    // per-band transmission (fs_update_direct_paths with one row; Params = nullptr: the defaults)
    fs_direct_path GetDirectPath(const fs_direct_params* Params = nullptr);

    bool bApplyReverb = true;   // .h:60

private:
    friend class AudioRayTracingSubsystem;
    friend class FrequenSeeAudioReverbPlugin;
    friend class FrequenSeeAudioSoundfieldReverbPlugin;
    friend class FrequenSeeAudioOcclusionPlugin;
    friend class FrequenSeeAudioReflectionPlugin;
    friend class FrequenSeeAudioBinauralPlugin;
    friend class FrequenSeeAudioAmbisonicPlugin;
    FVector Location_;
    AudioRayTracingSubsystem* SubSys_ = nullptr;
    fs_source Handle_ = -1;
};

class AudioRayTracingSubsystem {
public:
    static constexpr int USED_RAY_COUNT = 1000;   // AudioRayTracingSubsystem.h:176

    explicit AudioRayTracingSubsystem(int NumBands = 1, int Device = 0, int Rank = 0, int WorldSize = 1) {   // Initialize :32-36
        fs_config c;
        fs_config_default(&c);
        c.num_bands = NumBands; c.device = Device; c.rank = Rank; c.world_size = WorldSize;
        NumBands_ = NumBands;
        int rc = fs_context_create(&c, &Ctx_);
        if (rc != FS_OK) {
            std::string m = Ctx_ ? fs_last_error(Ctx_) : "fs_context_create failed";
            if (Ctx_) fs_context_destroy(Ctx_);
            Ctx_ = nullptr;
            throw std::runtime_error("FrequenSee: " + m);
        }
        fs_params_default(&Params);
        Params.num_rays = 2 * USED_RAY_COUNT;
    }
    ~AudioRayTracingSubsystem() { if (Ctx_) fs_context_destroy(Ctx_); }   // Deinitialize :38-42
    AudioRayTracingSubsystem(const AudioRayTracingSubsystem&) = delete;
    AudioRayTracingSubsystem& operator=(const AudioRayTracingSubsystem&) = delete;

    // RegisterGeometry / UnregisterGeometry (.h:99-100).  The first commit builds the tree on the host (binned SAH);
    // a registration change DURING play (Committed_ already) rebuilds it on the device instead, a tenth of the time
    // (fs_scene_commit_progressive: the SAH tree follows by itself from a background thread; RebuildQuality() forces it now).
    void RegisterGeometry(const AcousticGeometryComponent* Comp) { Geometry_.push_back(Comp); Dirty_ = true; }
    void UnregisterGeometry(const AcousticGeometryComponent* Comp) {
        for (size_t i = 0; i < Geometry_.size(); ++i)
            if (Geometry_[i] == Comp) { Geometry_.erase(Geometry_.begin() + (long)i); Dirty_ = true; break; }
    }
    void RebuildQuality() { Dirty_ = true; Committed_ = false; Commit(); }
    // Multi-GPU (one process per GPU, Rank / WorldSize given to the constructor): Id = the FS_COMM_ID_BYTES bytes rank 0
    // got from fs_comm_unique_id, shipped to every rank.  From then on every frame's energy buffer is summed over the
    // ranks inside the library and Commit() lets rank 0 build the tree for all.
    void CommInit(const void* Id) { Check(fs_comm_init(Ctx_, Id, FS_COMM_ID_BYTES)); }
    // One source per GPU (cfg5): no sharding, no reduce — a peer communicator only for GatherEnergy, after which any
    // rank can install a peer's histogram (UpdateEnergyBuffer on a mirror component) and serve its IR.
    void PeersInit(const void* Id, int Rank, int WorldSize) { Check(fs_peers_init(Ctx_, Id, FS_COMM_ID_BYTES, Rank, WorldSize)); Peers_ = WorldSize; }
    std::vector<float> GatherEnergy(fs_source Src) {             // [WorldSize][bands][bins], collective
        std::vector<float> Out((size_t)Peers_ * (size_t)NumBands_ * (size_t)fs_num_bins(Ctx_));
        Check(fs_gather_energy(Ctx_, Src, Out.data(), (int32_t)Out.size()));
        return Out;
    }
    // UAcousticMaterial table: Absorption [M][bands] (AcousticMaterial.h:22-30)
    void SetMaterials(const std::vector<float>& Absorption, int NumMaterials) {
        Absorption_ = Absorption; NumMaterials_ = NumMaterials; Dirty_ = true;
    }
    void RegisterSource(FrequenSeeAudioComponent* InComp) {      // .cpp:45-48
        Check(fs_source_create(Ctx_, &InComp->Handle_));
        InComp->SubSys_ = this;
        const FVector L = InComp->Location_;
        Check(fs_source_set_position(Ctx_, InComp->Handle_, &L.X));
        ActiveSources.push_back(InComp);
    }
    void UnRegisterSource(FrequenSeeAudioComponent* InComp) {    // .cpp:50-53
        for (size_t i = 0; i < ActiveSources.size(); ++i)
            if (ActiveSources[i] == InComp) {
                ActiveSources.erase(ActiveSources.begin() + (long)i);
                fs_source_destroy(Ctx_, InComp->Handle_);
                InComp->Handle_ = -1; InComp->SubSys_ = nullptr;
                break;
            }
    }
    void SetListenerLocation(FVector L) { Check(fs_listener_set_position(Ctx_, &L.X)); }   // PlayerPawn location :287

    // UpdateSource (.cpp:128-195): trace + evaluate + flush + deposit + reconstruct
    void UpdateSource(FrequenSeeAudioComponent& Src, std::vector<float>* EnergyOut = nullptr) {
        Commit();
        const int n = Src.NumBins() * NumBands();
        if (EnergyOut) EnergyOut->resize((size_t)n);
        Check(fs_compute_energy_response(Ctx_, Src.Handle_, &Params, EnergyOut ? EnergyOut->data() : nullptr));
        Check(fs_reconstruct_impulse_response(Ctx_, Src.Handle_, &Params));
    }
    // .cpp:883-886 — every active source; one batched frame on the device (fs_compute_energy_response_batch_async)
    void ForceUpdateSources() {
        if (ActiveSources.empty()) return;
        Commit();
        std::vector<fs_source> H;
        for (auto* s : ActiveSources) H.push_back(s->Handle_);
        Check(fs_update_sources(Ctx_, H.data(), (int32_t)H.size(), &Params));   // one batched frame, one reconstruct launch, one wait
    }
    // .cpp:55-85 (the caller drives every frame).  The reference draws from the engine's global rand() stream, so every
    // frame sees fresh samples: the seed advances.
    void Tick(float /*DeltaTime*/) {
        if (ActiveSources.empty()) return;
        if (Streamed_) {   // the reference's loop over the sources (.cpp:60-68), one pipelined launch per source
            Commit();
            for (auto* s : ActiveSources) {
                Check(fs_compute_energy_response_async(Ctx_, s->Handle_, &Params));
                Check(fs_reconstruct_impulse_response_async(Ctx_, s->Handle_, &Params));
            }
            Check(fs_submit(Ctx_));   // nothing waits: the IRs appear as they are published
        } else {
            ForceUpdateSources();
        }
        ++Params.seed;
    }
    // the direct sound of every active source in one launch: row i for ActiveSources[i] (fs_update_direct_paths; more than
    // FS_MAX_DIRECT_BATCH sources take one launch per FS_MAX_DIRECT_BATCH)
    std::vector<fs_direct_path> UpdateDirectPaths(const fs_direct_params* P = nullptr) {
        std::vector<fs_direct_path> Out(ActiveSources.size());
        if (Out.empty()) return Out;
        Commit();
        std::vector<fs_source> H;
        for (auto* s : ActiveSources) H.push_back(s->Handle_);
        for (size_t i = 0; i < H.size(); i += FS_MAX_DIRECT_BATCH)
            Check(fs_update_direct_paths(Ctx_, H.data() + i, (int32_t)std::min<size_t>(H.size() - i, FS_MAX_DIRECT_BATCH), P, Out.data() + i));
        return Out;
    }
    // The five rows-and-paths queries of every active source: Rows[i] and Paths[i * MaxPaths .. ) for ActiveSources[i]; MaxPaths =
    // P->max_paths, the default's without P; one call per FS_MAX_*_BATCH sources.
    // the first-order specular reflections (fs_update_reflection_paths)
    struct ReflectionPaths { int32_t MaxPaths = 0; std::vector<fs_reflection_row> Rows; std::vector<fs_reflection_path> Paths; };
    ReflectionPaths UpdateReflectionPaths(const fs_reflection_params* P = nullptr) {
        return UpdateRowsPaths<ReflectionPaths>(P, fs_reflection_params_default, fs_update_reflection_paths, FS_MAX_REFLECTIONS, FS_MAX_REFLECTION_BATCH);
    }
    // the first-order edge diffraction (fs_update_diffraction_paths)
    struct DiffractionPaths { int32_t MaxPaths = 0; std::vector<fs_diffraction_row> Rows; std::vector<fs_diffraction_path> Paths; };
    DiffractionPaths UpdateDiffractionPaths(const fs_diffraction_params* P = nullptr) {
        return UpdateRowsPaths<DiffractionPaths>(P, fs_diffraction_params_default, fs_update_diffraction_paths, FS_MAX_DIFFRACTIONS, FS_MAX_DIFFRACTION_BATCH);
    }
    // the second-order specular reflections (fs_update_reflection2_paths)
    struct Reflection2Paths { int32_t MaxPaths = 0; std::vector<fs_reflection2_row> Rows; std::vector<fs_reflection2_path> Paths; };
    Reflection2Paths UpdateReflection2Paths(const fs_reflection2_params* P = nullptr) {
        return UpdateRowsPaths<Reflection2Paths>(P, fs_reflection2_params_default, fs_update_reflection2_paths, FS_MAX_REFLECTION2_PATHS,
                                                 FS_MAX_REFLECTION2_BATCH);
    }
    // the diffraction round thick obstacles (fs_update_diffraction2_paths)
    struct Diffraction2Paths { int32_t MaxPaths = 0; std::vector<fs_diffraction2_row> Rows; std::vector<fs_diffraction2_path> Paths; };
    Diffraction2Paths UpdateDiffraction2Paths(const fs_diffraction2_params* P = nullptr) {
        return UpdateRowsPaths<Diffraction2Paths>(P, fs_diffraction2_params_default, fs_update_diffraction2_paths, FS_MAX_DIFFRACTION2_PATHS,
                                                  FS_MAX_DIFFRACTION2_BATCH);
    }
    // the paths off one reflector and round one edge (fs_update_mixed_paths)
    struct MixedPaths { int32_t MaxPaths = 0; std::vector<fs_mixed_row> Rows; std::vector<fs_mixed_path> Paths; };
    MixedPaths UpdateMixedPaths(const fs_mixed_params* P = nullptr) {
        return UpdateRowsPaths<MixedPaths>(P, fs_mixed_params_default, fs_update_mixed_paths, FS_MAX_MIXED_PATHS, FS_MAX_MIXED_BATCH);
    }
    // The probe graph (fs_pathing_*): Probes [count][3] in free air, the host's choice (a nav-mesh sample, a grid); the bake links
    // the pairs that see each other and returns the number of edges.  Bake again when PathingSceneChanged() says that a door has moved.
    int32_t SetPathingProbes(const std::vector<float>& Probes, const fs_pathing_bake_params* P = nullptr) {
        Check(fs_pathing_set_probes(Ctx_, Probes.data(), (int32_t)(Probes.size() / 3)));
        return Probes.size() < 3 ? 0 : BakePathing(P);
    }
    int32_t BakePathing(const fs_pathing_bake_params* P = nullptr) {
        Commit();
        Check(fs_pathing_bake(Ctx_, P));
        int32_t Edges = 0;
        Check(fs_pathing_info(Ctx_, nullptr, &Edges, nullptr, nullptr));
        return Edges;
    }
    bool PathingSceneChanged() const {
        int32_t Changed = 0;
        return fs_pathing_info(Ctx_, nullptr, nullptr, nullptr, &Changed) == FS_OK && Changed != 0;
    }
    // the route through the probe graph of every active source: row i for ActiveSources[i] (fs_update_pathing_paths)
    std::vector<fs_pathing_path> UpdatePathingPaths(const fs_pathing_params* P = nullptr) {
        std::vector<fs_pathing_path> Out(ActiveSources.size());
        if (Out.empty()) return Out;
        Commit();
        std::vector<fs_source> H;
        for (auto* s : ActiveSources) H.push_back(s->Handle_);
        for (size_t i = 0; i < H.size(); i += FS_MAX_PATHING_BATCH)
            Check(fs_update_pathing_paths(Ctx_, H.data() + i, (int32_t)std::min<size_t>(H.size() - i, FS_MAX_PATHING_BATCH), P, Out.data() + i));
        return Out;
    }
private:
    template <typename Result, typename Params, typename Row, typename Path>
    Result UpdateRowsPaths(const Params* P, void (*Defaults)(Params*), int (*Update)(fs_context*, const fs_source*, int32_t, const Params*, Row*, Path*),
                           int MaxPathsCap, size_t Batch) {
        Params Def;
        Defaults(&Def);
        Result Out;
        Out.MaxPaths = P ? P->max_paths : Def.max_paths;
        if (ActiveSources.empty()) return Out;
        Out.Rows.resize(ActiveSources.size());
        Out.Paths.resize(ActiveSources.size() * (size_t)std::min(std::max(Out.MaxPaths, 1), MaxPathsCap));   // (a bad max_paths is refused below)
        Commit();
        std::vector<fs_source> H;
        for (auto* s : ActiveSources) H.push_back(s->Handle_);
        for (size_t i = 0; i < H.size(); i += Batch)
            Check(Update(Ctx_, H.data() + i, (int32_t)std::min(H.size() - i, Batch), P, Out.Rows.data() + i, Out.Paths.data() + i * (size_t)Out.MaxPaths));
        return Out;
    }
public:
    // fs_set_pipelining (0 off, 1, 2): Tick streams the sources instead of batching them
    void SetPipelining(int Depth) { Check(fs_set_pipelining(Ctx_, Depth)); Streamed_ = Depth != 0; }
    // fs_set_frames_per_launch (1 .. 4): consecutive streamed frames share a launch (each keeps its seed, buffer and IR)
    void SetFramesPerLaunch(int N) { Check(fs_set_frames_per_launch(Ctx_, N)); }
    void Synchronize() { Check(fs_synchronize(Ctx_)); }

    int NumBands() const { return NumBands_; }
    fs_context* Context() const { return Ctx_; }
    void Commit() {
        if (!Dirty_) return;
        std::vector<float> xyz; std::vector<uint16_t> mat; std::vector<uint32_t> obj;
        for (const auto* g : Geometry_) {
            xyz.insert(xyz.end(), g->Triangles.begin(), g->Triangles.end());
            mat.insert(mat.end(), g->MaterialId.begin(), g->MaterialId.end());
            obj.insert(obj.end(), g->MaterialId.size(), g->Actor);
        }
        Check(fs_scene_set_triangles(Ctx_, xyz.data(), mat.data(), (int32_t)mat.size()));
        Check(fs_scene_set_materials(Ctx_, Absorption_.data(), nullptr, nullptr, NumMaterials_,
                                     NumMaterials_ ? (int32_t)(Absorption_.size() / (size_t)NumMaterials_) : NumBands()));
        Check(fs_scene_set_objects(Ctx_, obj.data(), (int32_t)obj.size()));
        Check(Committed_ ? fs_scene_commit_progressive(Ctx_) : fs_scene_commit(Ctx_));
        Dirty_ = false;
        Committed_ = true;
    }
    // A registered geometry component moved (ECC_WorldDynamic prop): its triangles are rewritten in place and the
    // acceleration structure is refitted on the device before the next trace — no rebuild.  `Comp->Triangles`
    // already holds the new world-space positions; the triangle count must not change.
    void GeometryMoved(const AcousticGeometryComponent* Comp) {
        Commit();
        size_t first = 0;
        for (const auto* g : Geometry_) {
            if (g == Comp) {
                Check(fs_scene_update_triangles(Ctx_, (int32_t)first, (int32_t)g->MaterialId.size(), g->Triangles.data()));
                return;
            }
            first += g->MaterialId.size();
        }
        throw std::runtime_error("FrequenSee: geometry component is not registered");
    }
    // The same for a mover the engine describes by its component transform: M = row-major 3 x 4 {r00 r01 r02 tx, ...} applied
    // to the triangles the component REGISTERED (`Comp->Triangles` stays the rest mesh and is not read here).  Absolute, not
    // cumulative; 48 bytes, no upload of vertices and no wait.  The component's Actor id must be its own.
    void GeometryMoved(const AcousticGeometryComponent* Comp, const float M[12]) {
        Commit();
        const uint32_t Id = Comp->Actor;
        Check(fs_scene_set_object_transforms(Ctx_, &Id, M, 1));
    }
    void Check(int rc) const { if (rc != FS_OK) throw std::runtime_error(std::string("FrequenSee: ") + fs_last_error(Ctx_)); }

    fs_params Params;                                   // the constants of AudioRayTracingSubsystem.cpp:282-284, 362-413
    std::vector<FrequenSeeAudioComponent*> ActiveSources;

private:
    fs_context* Ctx_ = nullptr;
    std::vector<const AcousticGeometryComponent*> Geometry_;
    std::vector<float> Absorption_;
    int NumMaterials_ = 0;
    bool Dirty_ = true;
    bool Committed_ = false;
    int NumBands_ = 1;
    int Peers_ = 0;
    bool Streamed_ = false;
    friend class FrequenSeeAudioComponent;
    friend class MaterialAcousticProcessor;
    friend class FrequenSeeAudioReverbPlugin;
    friend class FrequenSeeAudioSoundfieldReverbPlugin;
    friend class FrequenSeeAudioOcclusionPlugin;
    friend class FrequenSeeAudioReflectionPlugin;
    friend class FrequenSeeAudioBinauralPlugin;
    friend class FrequenSeeAudioAmbisonicPlugin;
};

inline FrequenSeeAudioComponent::~FrequenSeeAudioComponent() { OnUnregister(); }
inline void FrequenSeeAudioComponent::OnRegister(AudioRayTracingSubsystem& S) { S.RegisterSource(this); }
inline void FrequenSeeAudioComponent::OnUnregister() { if (SubSys_) SubSys_->UnRegisterSource(this); }
inline void FrequenSeeAudioComponent::SetComponentLocation(FVector L) {
    Location_ = L;
    if (SubSys_) SubSys_->Check(fs_source_set_position(SubSys_->Ctx_, Handle_, &L.X));
}
inline void FrequenSeeAudioComponent::SetForwardVector(FVector F) {
    SubSys_->Check(fs_source_set_orientation(SubSys_->Ctx_, Handle_, &F.X));
}
inline void FrequenSeeAudioComponent::SetDirectivity(const std::vector<float>& Gains, int Samples) {
    if (Gains.empty()) { SubSys_->Check(fs_source_set_directivity(SubSys_->Ctx_, Handle_, nullptr, 0, 0)); return; }
    const int Bands = Samples > 0 ? (int)(Gains.size() / (size_t)Samples) : 0;
    SubSys_->Check(fs_source_set_directivity(SubSys_->Ctx_, Handle_, Gains.data(), Bands, Samples));
}
inline void FrequenSeeAudioComponent::SetOrderWindow(int MinOrder, int MaxOrder) {
    SubSys_->Check(fs_source_set_order_window(SubSys_->Ctx_, Handle_, (int32_t)MinOrder, (int32_t)MaxOrder));
}
inline void FrequenSeeAudioComponent::GetOrderWindow(int& MinOrder, int& MaxOrder) const {
    int32_t Lo = 0, Hi = 0;
    SubSys_->Check(fs_source_get_order_window(SubSys_->Ctx_, Handle_, &Lo, &Hi));
    MinOrder = (int)Lo; MaxOrder = (int)Hi;
}
inline int FrequenSeeAudioComponent::NumBins() const { return fs_num_bins(SubSys_->Ctx_); }
inline int FrequenSeeAudioComponent::NumSamples() const { return fs_num_samples(SubSys_->Ctx_); }
inline void FrequenSeeAudioComponent::FlushEnergyBuffer() { SubSys_->Check(fs_flush_energy_buffer(SubSys_->Ctx_, Handle_)); }
inline void FrequenSeeAudioComponent::UpdateEnergyBuffer(const std::vector<float>& V) {
    SubSys_->Check(fs_update_energy_buffer(SubSys_->Ctx_, Handle_, V.data(), (int32_t)V.size()));
}
inline void FrequenSeeAudioComponent::AddEnergyAtDelay(float D, float E, int Band) {
    SubSys_->Check(fs_add_energy_at_delay(SubSys_->Ctx_, Handle_, Band, D, E));
}
inline std::vector<float> FrequenSeeAudioComponent::EnergyBuffer() const {
    std::vector<float> v((size_t)NumBins() * (size_t)SubSys_->NumBands());
    SubSys_->Check(fs_get_energy_buffer(SubSys_->Ctx_, Handle_, v.data(), (int32_t)v.size()));
    return v;
}
inline void FrequenSeeAudioComponent::ReconstructImpulseResponse() {
    SubSys_->Check(fs_reconstruct_impulse_response(SubSys_->Ctx_, Handle_, &SubSys_->Params));
}
inline const float* FrequenSeeAudioComponent::GetImpulseResponse(int Channel, int* N) const {
    const float* p = nullptr;
    int32_t n = 0;
    SubSys_->Check(fs_get_impulse_response(SubSys_->Ctx_, Handle_, Channel, &p, &n));
    if (N) *N = n;
    return p;
}
inline float FrequenSeeAudioComponent::GetOcclusionAttenuation() const {
    float v = 1.f;
    SubSys_->Check(fs_get_occlusion_attenuation(SubSys_->Ctx_, Handle_, &v));
    return v;
}
inline fs_sound_result FrequenSeeAudioComponent::UpdateSound(uint64_t Seed) {
    SubSys_->Commit();
    fs_sound_params p;
    fs_sound_params_default(&p);
    p.seed = Seed;
    fs_sound_result r{};
    SubSys_->Check(fs_update_sound(SubSys_->Ctx_, Handle_, &p, &r));
    return r;
}
inline void FrequenSeeAudioComponent::SetImpulseResponse(const std::vector<float>& IR) {
    SubSys_->Check(fs_set_impulse_response(SubSys_->Ctx_, Handle_, IR.data(), (int32_t)IR.size()));
}
inline std::vector<float> FrequenSeeAudioComponent::GenerateDummyImpulseResponse() {
    std::vector<float> IR((size_t)fs_num_samples(SubSys_->Ctx_), 0.0f);
    if (!IR.empty()) { IR.front() = 1.0f; IR.back() = 1.0f; }
    SetImpulseResponse(IR);
    return IR;
}
inline std::vector<fs_room_parameters> FrequenSeeAudioComponent::GetRoomParameters(uint64_t* Sequence) const {
    std::vector<fs_room_parameters> v((size_t)SubSys_->NumBands());
    uint64_t seq = 0;
    SubSys_->Check(fs_get_room_parameters(SubSys_->Ctx_, Handle_, v.data(), (int32_t)v.size(), &seq));
    if (Sequence) *Sequence = seq;
    if (seq == 0) v.clear();
    return v;
}
inline fs_direct_path FrequenSeeAudioComponent::GetDirectPath(const fs_direct_params* Params) {
    SubSys_->Commit();
    fs_direct_path r{};
    SubSys_->Check(fs_update_direct_paths(SubSys_->Ctx_, &Handle_, 1, Params, &r));
    return r;
}
inline void FrequenSeeAudioComponent::SaveImpulseResponse(const std::string& Path, int Channel) const {
    SubSys_->Check(fs_save_impulse_response(SubSys_->Ctx_, Handle_, Channel, Path.c_str()));
}

// FMaterialAcousticFD / FAcousticOutputs (Public/MaterialAcousticProcessor.h:24-53)
struct MaterialAcousticFD {
    std::vector<float> Absorption, Transmission, Scattering;   // each N/2 + 1 responses
};
struct AcousticOutputs {
    std::vector<float> Specular, Diffuse, Transmitted;
};

class MaterialAcousticProcessor {
public:
    explicit MaterialAcousticProcessor(AudioRayTracingSubsystem& SubSys) : SubSys_(&SubSys) {}
    // ApplyMaterialFD (MaterialAcousticProcessor.cpp:8-107).  A wrong curve length logs an error and returns
    // empty outputs in the reference (:20-26); here it throws with the same message.
    AcousticOutputs ApplyMaterialFD(const std::vector<float>& InBuffer, const MaterialAcousticFD& Props) const {
        AcousticOutputs Out;
        const size_t L = InBuffer.size();
        if (Props.Absorption.size() != Props.Transmission.size() || Props.Absorption.size() != Props.Scattering.size())
            throw std::runtime_error("FrequenSee: response curves differ in length");
        Out.Specular.resize(L); Out.Diffuse.resize(L); Out.Transmitted.resize(L);
        SubSys_->Check(fs_apply_material_fd(SubSys_->Ctx_, InBuffer.data(), (int32_t)L, Props.Absorption.data(),
                                            Props.Transmission.data(), Props.Scattering.data(),
                                            (int32_t)Props.Absorption.size(), Out.Specular.data(), Out.Diffuse.data(),
                                            Out.Transmitted.data()));
        return Out;
    }

private:
    AudioRayTracingSubsystem* SubSys_;
};

// FFrequenSeeAudioReverbPlugin (Private/FrequenSeeAudioReverbPlugin.cpp:74-213): per audio callback every source's block is
// convolved with its impulse response — fs_reverb_process_batch, one call for all sources.  Not in the reference: Engine (the
// partitioned FFT engine) and Ears, a two-ear late field with the interaural coherence of a diffuse field (SetEars installs the
// context's ear set; a source gets ears at its OnInitSource, which then also selects the partitioned engine).
class FrequenSeeAudioReverbPlugin {
public:
    int FrameSize = 1024;   // AudioCallbackBufferFrameSize, Config/DefaultEngine.ini:13
    int Engine = FS_REVERB_ENGINE_DIRECT;
    bool Ears = false;
    explicit FrequenSeeAudioReverbPlugin(AudioRayTracingSubsystem& SubSys) : SubSys_(&SubSys) {}
    void Initialize(int BufferLength = 1024) { FrameSize = BufferLength; }
    void SetEars(float RadiusCm = FS_HRTF_DEFAULT_RADIUS_CM, float SoundSpeedCmS = FS_HRTF_DEFAULT_SOUND_SPEED_CM_S) {
        fs_reverb_ears_desc D;
        fs_reverb_ears_default(&D);
        D.radius_cm = RadiusCm; D.sound_speed_cm_s = SoundSpeedCmS;
        SubSys_->Check(fs_reverb_ears_set(SubSys_->Ctx_, &D));
        Ears = true;
    }
    void OnInitSource(const FrequenSeeAudioComponent& C) {
        SubSys_->Check(fs_reverb_set_engine(SubSys_->Ctx_, C.Handle_, Ears ? FS_REVERB_ENGINE_PARTITIONED : Engine));
        SubSys_->Check(fs_reverb_set_ears(SubSys_->Ctx_, C.Handle_, Ears ? 1 : 0));
        SubSys_->Check(fs_reverb_init(SubSys_->Ctx_, C.Handle_, FrameSize));
    }
    void OnReleaseSource(const FrequenSeeAudioComponent& C) { SubSys_->Check(fs_reverb_release(SubSys_->Ctx_, C.Handle_)); }
    // In [count][FrameSize * 2] interleaved stereo, row i for Sources[i]; Out [count][FrameSize * 2] or nullptr, Mix [FrameSize * 2] or nullptr
    void ProcessAudio(const std::vector<FrequenSeeAudioComponent*>& Sources, const float* In, float* Out, float* Mix = nullptr) {
        std::vector<fs_source> H;
        std::vector<int32_t> On;
        for (const auto* s : Sources) { H.push_back(s->Handle_); On.push_back(s->bApplyReverb ? 1 : 0); }
        SubSys_->Check(fs_reverb_process_batch(SubSys_->Ctx_, H.data(), (int32_t)H.size(), In, Out, On.data(), 0u, Mix));
    }
    // h_L and h_R of the source's newest impulse response, for a host with a convolver of its own
    void EarImpulseResponses(const FrequenSeeAudioComponent& C, std::vector<float>& Left, std::vector<float>& Right) const {
        const int n = fs_num_samples(SubSys_->Ctx_);
        Left.assign((size_t)n, 0.0f); Right.assign((size_t)n, 0.0f);
        SubSys_->Check(fs_reverb_copy_ear_impulse_responses(SubSys_->Ctx_, C.Handle_, Left.data(), Right.data(), n));
    }

protected:
    AudioRayTracingSubsystem* SubSys_;
};

// Not in the reference: the reverb plugin with the late field on an ambisonic bus of (Order + 1)^2 channels, ACN order and SN3D
// normalisation — fs_reverb_soundfield_process_batch, the diffuse counterpart of FrequenSeeAudioAmbisonicPlugin's voices, whose Mix
// it is summed with.  SetOrder installs the context's carrier set; OnInitSource selects the partitioned engine and the soundfield.
// The output is not clamped and bApplyReverb is not read: the call has no bypass row.
class FrequenSeeAudioSoundfieldReverbPlugin : public FrequenSeeAudioReverbPlugin {
public:
    int Order = 1;   // 0 .. FS_MAX_AMBISONIC_ORDER; SetOrder before OnInitSource
    explicit FrequenSeeAudioSoundfieldReverbPlugin(AudioRayTracingSubsystem& SubSys) : FrequenSeeAudioReverbPlugin(SubSys) {}
    int Channels() const { return (Order + 1) * (Order + 1); }
    void SetOrder(int NewOrder = 1) {
        SubSys_->Check(fs_reverb_soundfield_set(SubSys_->Ctx_, NewOrder));
        Order = NewOrder;
    }
    void OnInitSource(const FrequenSeeAudioComponent& C) {
        SubSys_->Check(fs_reverb_set_engine(SubSys_->Ctx_, C.Handle_, FS_REVERB_ENGINE_PARTITIONED));
        SubSys_->Check(fs_reverb_set_ears(SubSys_->Ctx_, C.Handle_, 0));
        SubSys_->Check(fs_reverb_set_soundfield(SubSys_->Ctx_, C.Handle_, 1));
        SubSys_->Check(fs_reverb_init(SubSys_->Ctx_, C.Handle_, FrameSize));
    }
    // In [count][FrameSize * 2] interleaved stereo, row i for Sources[i]; Out [count][FrameSize * Channels()] or nullptr,
    // Mix [FrameSize * Channels()] or nullptr: element s * Channels() + c
    void ProcessAudio(const std::vector<FrequenSeeAudioComponent*>& Sources, const float* In, float* Out, float* Mix = nullptr) {
        std::vector<fs_source> H;
        for (const auto* s : Sources) H.push_back(s->Handle_);
        SubSys_->Check(fs_reverb_soundfield_process_batch(SubSys_->Ctx_, H.data(), (int32_t)H.size(), In, Out, 0u, Mix));
    }
    // h_c [Channels()][fs_num_samples] of the source's newest impulse response, for a host with a convolver of its own
    void ImpulseResponses(const FrequenSeeAudioComponent& C, std::vector<float>& Irs) const {
        const int n = fs_num_samples(SubSys_->Ctx_);
        Irs.assign((size_t)Channels() * (size_t)n, 0.0f);
        SubSys_->Check(fs_reverb_copy_soundfield_impulse_responses(SubSys_->Ctx_, C.Handle_, Irs.data(), n));
    }
};

// What the two render plugins below share: the shape of their callback and a path's arrival time as the delay of a target or a voice
class FrequenSeeRenderPlugin {
public:
    int FrameSize = 1024;   // AudioCallbackBufferFrameSize, Config/DefaultEngine.ini:13
    int Taps = 255;
    float MaxDelaySeconds = 1.0f;
    int SampleRate = 48000;   // fs_config_default's, FSAC.h:133

protected:
    explicit FrequenSeeRenderPlugin(AudioRayTracingSubsystem& SubSys) : SubSys_(&SubSys) {}
    // the arrival time less the filter's own latency of (Taps - 1) / 2 samples, not below 0
    float TargetDelay(float Arrival) const { return (float)std::max((double)Arrival - (double)((Taps - 1) / 2) / (double)SampleRate, 0.0); }
    AudioRayTracingSubsystem* SubSys_;
};

// FFrequenSeeAudioOcclusionPlugin (Private/FrequenSeeAudioOcclusionPlugin.cpp:33-50) with the multiply the reference leaves
// commented out done: per audio callback every source's block is delayed by its direct path's arrival time (a fractional,
// slew-limited delay: the Doppler shift) and filtered by its per-band transmission — fs_direct_render_process_batch, one call
// for all sources.  Distance attenuation stays the host's.
class FrequenSeeAudioOcclusionPlugin : public FrequenSeeRenderPlugin {
public:
    explicit FrequenSeeAudioOcclusionPlugin(AudioRayTracingSubsystem& SubSys) : FrequenSeeRenderPlugin(SubSys) {}
    void Initialize(int BufferLength = 1024, int TapCount = 255, float MaxDelay = 1.0f) {
        FrameSize = BufferLength; Taps = TapCount; MaxDelaySeconds = MaxDelay;
    }
    void OnInitSource(const FrequenSeeAudioComponent& C) {
        SubSys_->Check(fs_direct_render_init(SubSys_->Ctx_, C.Handle_, FrameSize, Taps, MaxDelaySeconds));
    }
    void OnReleaseSource(const FrequenSeeAudioComponent& C) { SubSys_->Check(fs_direct_render_release(SubSys_->Ctx_, C.Handle_)); }
    // the callback's targets from UpdateDirectPaths rows: band_gain = transmission, delay = TargetDelay of the path's arrival time
    std::vector<fs_direct_render_target> Targets(const std::vector<fs_direct_path>& Paths) const {
        std::vector<fs_direct_render_target> T(Paths.size());
        for (size_t i = 0; i < Paths.size(); ++i) {
            T[i].delay = TargetDelay(Paths[i].delay);
            for (int b = 0; b < FS_MAX_BANDS; ++b) T[i].band_gain[b] = Paths[i].transmission[b];
        }
        return T;
    }
    // In [count][FrameSize * 2] interleaved stereo, row i for Sources[i] and Paths[i]; Out [count][FrameSize * 2] or nullptr,
    // Mix [FrameSize * 2] (the fp32 sum of the rows in list order) or nullptr
    void ProcessAudio(const std::vector<FrequenSeeAudioComponent*>& Sources, const float* In, const std::vector<fs_direct_path>& Paths,
                      float* Out, float* Mix = nullptr) {
        std::vector<fs_source> H;
        for (const auto* s : Sources) H.push_back(s->Handle_);
        const std::vector<fs_direct_render_target> T = Targets(Paths);
        if (T.size() != H.size()) throw std::runtime_error("FrequenSee: one direct path per source");
        SubSys_->Check(fs_direct_render_process_batch(SubSys_->Ctx_, H.data(), (int32_t)H.size(), In, T.data(), Out, Mix));
    }
};

// Not in the reference: per audio callback every source's block is rendered once per first-order reflection of
// fs_update_reflection_paths — delayed by the path's arrival time (fractional and slew-limited: each reflection has a Doppler shift
// of its own), filtered by its per-band reflectance, weighted by a per-channel gain and summed — fs_reflection_render_process_batch,
// one call for all sources.  A reflection is recognised from callback to callback by its triangle; one that appears or vanishes
// fades over one block.  Panning and the distance law are this plugin's (Voices), not the library's.
class FrequenSeeAudioReflectionPlugin : public FrequenSeeRenderPlugin {
public:
    explicit FrequenSeeAudioReflectionPlugin(AudioRayTracingSubsystem& SubSys) : FrequenSeeRenderPlugin(SubSys) {}
    void Initialize(int BufferLength = 1024, int TapCount = 255, int Voices = FS_MAX_REFLECTION_VOICES, float MaxDelay = 1.0f) {
        FrameSize = BufferLength; Taps = TapCount; VoiceCount = Voices; MaxDelaySeconds = MaxDelay;
    }
    void OnInitSource(const FrequenSeeAudioComponent& C) {
        SubSys_->Check(fs_reflection_render_init(SubSys_->Ctx_, C.Handle_, FrameSize, Taps, VoiceCount, MaxDelaySeconds));
    }
    void OnReleaseSource(const FrequenSeeAudioComponent& C) { SubSys_->Check(fs_reflection_render_release(SubSys_->Ctx_, C.Handle_)); }
    // one source's entries from its row and paths of fs_update_reflection_paths, over the first Row.returned paths: key = triangle,
    // band_gain = reflectance, delay = TargetDelay of the path's arrival time.
    // channel_gain = (1, 1); with Right (the listener's unit right vector) the constant-power pan (cos t, sin t),
    // t = (dot(direction, Right) + 1) pi / 4; with ReferenceLength > 0 (cm) scaled by min(1, ReferenceLength / length).
    // DRow / DPaths (the same source's row and paths of fs_update_diffraction_paths) append one voice per returned diffraction path:
    // band_gain = gain, delay, pan and distance law as above, key = 0x80000000 | (4 triangle + edge) — no reflection's key while the
    // scene has fewer than 2^29 triangles; an index beyond that is refused.  SRow / SPaths (the same source's row and paths of
    // fs_update_reflection2_paths) append one voice per returned second-order path: band_gain = reflectance, delay, pan and distance
    // law as above, key = SecondOrderKey(a, b).  Two second-order paths of the row whose keys collide: the earlier in the row — the
    // shorter, ties by (a, b) — is kept and the other dropped (the renderer refuses duplicate keys).  TRow / TPaths (the same
    // source's row and paths of fs_update_diffraction2_paths) append, last, one voice per returned path round two edges: band_gain =
    // gain, key = Diffraction2Key(triangle, edge); on colliding keys the earlier in the row is kept likewise.  MRow / MPaths (the
    // same source's row and paths of fs_update_mixed_paths) append, after those, one voice per returned path off a reflector and
    // round an edge: band_gain = gain, key = MixedKey(triangle, edge, end), colliding keys likewise; with them a diffraction path's
    // triangle must stay below 2^28, or its key would reach the mixed paths' range
    static uint32_t SecondOrderKey(uint32_t A, uint32_t B) { return 0x40000000u | ((A * 2654435761u + B) >> 2); }
    static uint32_t Diffraction2Key(const uint32_t (&Triangle)[2], const uint32_t (&Edge)[2]) {
        return 0x20000000u | (((4u * Triangle[0] + Edge[0]) * 2654435761u + (4u * Triangle[1] + Edge[1])) >> 3);
    }
    static uint32_t MixedKey(const uint32_t (&Triangle)[2], uint32_t Edge, uint32_t End) {
        return 0xC0000000u | ((Triangle[0] * 2654435761u + 4u * (2u * (4u * Triangle[1] + Edge) + End)) >> 2);
    }
    std::vector<fs_reflection_voice> Voices(const fs_reflection_row& Row, const fs_reflection_path* Paths, const FVector* Right = nullptr,
                                            float ReferenceLength = 0.0f, const fs_diffraction_row* DRow = nullptr,
                                            const fs_diffraction_path* DPaths = nullptr, const fs_reflection2_row* SRow = nullptr,
                                            const fs_reflection2_path* SPaths = nullptr, const fs_diffraction2_row* TRow = nullptr,
                                            const fs_diffraction2_path* TPaths = nullptr, const fs_mixed_row* MRow = nullptr,
                                            const fs_mixed_path* MPaths = nullptr) const {
        std::vector<fs_reflection_voice> V;
        ForEachVoice(Row, Paths, DRow, DPaths, SRow, SPaths, TRow, TPaths, MRow, MPaths,
                     [&](uint32_t Key, float Delay, const float* Gain, const float* Dir, float Length) {
                         V.push_back(Voice(Key, Delay, Gain, Dir, Length, Right, ReferenceLength));
                     });
        return V;
    }
    // what Voices keeps of a source's path records, in its order: Fn(key, arrival time, band gains, arrival direction, length) per
    // voice, with the keys, their range checks and the dropping of colliding keys as described above
    template <class F>
    void ForEachVoice(const fs_reflection_row& Row, const fs_reflection_path* Paths, const fs_diffraction_row* DRow, const fs_diffraction_path* DPaths,
                      const fs_reflection2_row* SRow, const fs_reflection2_path* SPaths, const fs_diffraction2_row* TRow,
                      const fs_diffraction2_path* TPaths, const fs_mixed_row* MRow, const fs_mixed_path* MPaths, F&& Fn) const {
        const size_t NR = (size_t)Row.returned, ND = DRow && DPaths ? (size_t)DRow->returned : 0, NS = SRow && SPaths ? (size_t)SRow->returned : 0;
        const size_t NT = TRow && TPaths ? (size_t)TRow->returned : 0, NM = MRow && MPaths ? (size_t)MRow->returned : 0;
        std::vector<uint32_t> Keys;   // of the voices kept so far
        Keys.reserve(NR + ND + NS + NT + NM);
        for (size_t i = 0; i < NR + ND + NS + NT + NM; ++i) {
            if (i >= NR + ND + NS + NT) {   // a mixed path: every field it needs under one name
                const fs_mixed_path& M = MPaths[i - NR - ND - NS - NT];
                const uint32_t Key = MixedKey(M.triangle, M.edge, M.end);
                if (std::find(Keys.begin() + (std::ptrdiff_t)(NR + ND), Keys.end(), Key) != Keys.end()) continue;
                Keys.push_back(Key);
                Fn(Key, M.delay, M.gain, M.direction, M.length);
                continue;
            }
            const bool Refl = i < NR, Second = i >= NR + ND && i < NR + ND + NS, Thick = i >= NR + ND + NS;
            const fs_reflection2_path* S = Second ? SPaths + (i - NR - ND) : nullptr;
            const fs_diffraction2_path* T = Thick ? TPaths + (i - NR - ND - NS) : nullptr;
            const uint32_t Tri = Refl ? Paths[i].triangle : (Second || Thick ? 0u : DPaths[i - NR].triangle);
            if ((ND || (SRow && SPaths) || (TRow && TPaths)) && Tri >= (0x80000000u >> 2))
                throw std::runtime_error("FrequenSee: triangle index 2^29 or above: the keys of the path kinds would collide");
            if (MRow && MPaths && !Refl && !Second && !Thick && Tri >= (0x80000000u >> 3))
                throw std::runtime_error("FrequenSee: a diffraction path's triangle index is 2^28 or above: its key would collide with the mixed paths' keys");
            const float* Dir = Refl ? Paths[i].direction : (Second ? S->direction : (Thick ? T->direction : DPaths[i - NR].direction));
            const float* Gain = Refl ? Paths[i].reflectance : (Second ? S->reflectance : (Thick ? T->gain : DPaths[i - NR].gain));
            const float Delay = Refl ? Paths[i].delay : (Second ? S->delay : (Thick ? T->delay : DPaths[i - NR].delay));
            const float Length = Refl ? Paths[i].length : (Second ? S->length : (Thick ? T->length : DPaths[i - NR].length));
            const uint32_t Key = Refl ? Tri : (Second ? SecondOrderKey(S->triangle[0], S->triangle[1])
                                                      : (Thick ? Diffraction2Key(T->triangle, T->edge) : (0x80000000u | (Tri * 4u + DPaths[i - NR].edge))));
            if ((Second || Thick) && std::find(Keys.begin() + (std::ptrdiff_t)(NR + ND), Keys.end(), Key) != Keys.end()) continue;
            Keys.push_back(Key);
            Fn(Key, Delay, Gain, Dir, Length);
        }
    }
    // The voice of a source's row of UpdatePathingPaths, appended by the host to what Voices returned: true and *Out filled iff the
    // row is FS_PATHING_FOUND and not FS_PATHING_DIRECT (a source in plain sight is spoken for by the direct sound and the early
    // paths).  key = FS_PATHING_VOICE_KEY (0x80000003: no diffraction key, whose low bits are an edge 0 .. 2), band_gain = gain,
    // delay, pan (from `direction`, towards the first probe) and distance law as a diffraction path's
    bool PathingVoice(const fs_pathing_path& P, fs_reflection_voice* Out, const FVector* Right = nullptr, float ReferenceLength = 0.0f) const {
        if ((P.flags & (FS_PATHING_FOUND | FS_PATHING_DIRECT)) != FS_PATHING_FOUND) return false;
        *Out = Voice(FS_PATHING_VOICE_KEY, P.delay, P.gain, P.direction, P.length, Right, ReferenceLength);
        return true;
    }
    // one voice: the key, the target delay, the band gains, and the pan and distance law of Voices
    fs_reflection_voice Voice(uint32_t Key, float Delay, const float* Gain, const float* Dir, float Length, const FVector* Right,
                              float ReferenceLength) const {
        fs_reflection_voice V{};
        V.key = Key;
        V.delay = TargetDelay(Delay);
        for (int b = 0; b < FS_MAX_BANDS; ++b) V.band_gain[b] = Gain[b];
        double L = 1.0, R = 1.0;
        if (Right) {
            const double Dot = (double)Dir[0] * Right->X + (double)Dir[1] * Right->Y + (double)Dir[2] * Right->Z;
            const double T = (Dot + 1.0) * 3.14159265358979323846 / 4.0;
            L = std::cos(T); R = std::sin(T);
        }
        if (ReferenceLength > 0.0f) {
            const double G = std::min(1.0, (double)ReferenceLength / (double)Length);
            L *= G; R *= G;
        }
        V.channel_gain[0] = (float)L;
        V.channel_gain[1] = (float)R;
        return V;
    }
    // In [count][FrameSize * 2] interleaved stereo, row i for Sources[i], Rows[i] and Paths[i * MaxPaths ..] (the arrays
    // fs_update_reflection_paths filled with max_paths = MaxPaths); Out [count][FrameSize * 2] or nullptr, Mix [FrameSize * 2] (the
    // fp32 sum of the rows in list order) or nullptr, Counts [count] or nullptr; Diffraction = UpdateDiffractionPaths' result for the
    // same sources (its voices follow each source's reflections) or nullptr; Second = UpdateReflection2Paths' result for the same
    // sources (its voices follow those) or nullptr; Thick = UpdateDiffraction2Paths' result for the same sources (its voices come
    // after those) or nullptr; Mixed = UpdateMixedPaths' result for the same sources (its voices come last) or nullptr.  A source's
    // table has MaxPaths + Diffraction->MaxPaths + Second->MaxPaths + Thick->MaxPaths + Mixed->MaxPaths entries,
    // FS_MAX_REFLECTION_VOICES (32) at most: the first four defaults of 8, 4, 16 and 4 fit, with the mixed paths' 8 a host lowers one
    // of them; 16 + 16 + 16 is refused
    void ProcessAudio(const std::vector<FrequenSeeAudioComponent*>& Sources, const float* In, const std::vector<fs_reflection_row>& Rows,
                      const std::vector<fs_reflection_path>& Paths, int MaxPaths, float* Out, float* Mix = nullptr,
                      const FVector* Right = nullptr, float ReferenceLength = 0.0f, fs_reflection_render_row* Counts = nullptr,
                      const AudioRayTracingSubsystem::DiffractionPaths* Diffraction = nullptr,
                      const AudioRayTracingSubsystem::Reflection2Paths* Second = nullptr,
                      const AudioRayTracingSubsystem::Diffraction2Paths* Thick = nullptr,
                      const AudioRayTracingSubsystem::MixedPaths* Mixed = nullptr) {
        const int DMax = Diffraction ? Diffraction->MaxPaths : 0, SMax = Second ? Second->MaxPaths : 0, TMax = Thick ? Thick->MaxPaths : 0;
        const int MMax = Mixed ? Mixed->MaxPaths : 0;
        const int Stride = MaxPaths + DMax + SMax + TMax + MMax;
        if (Stride > FS_MAX_REFLECTION_VOICES)
            throw std::runtime_error("FrequenSee: max_paths of the reflections, the diffraction paths and the second-order paths add up to " +
                                     std::to_string(Stride) + " voices per source, more than FS_MAX_REFLECTION_VOICES");
        if (Rows.size() != Sources.size() || Paths.size() != Sources.size() * (size_t)MaxPaths || MaxPaths < 1 || DMax < 0 || SMax < 0 || TMax < 0 || MMax < 0 ||
            (Diffraction && (Diffraction->Rows.size() != Sources.size() || Diffraction->Paths.size() != Sources.size() * (size_t)DMax)) ||
            (Second && (Second->Rows.size() != Sources.size() || Second->Paths.size() != Sources.size() * (size_t)SMax)) ||
            (Thick && (Thick->Rows.size() != Sources.size() || Thick->Paths.size() != Sources.size() * (size_t)TMax)) ||
            (Mixed && (Mixed->Rows.size() != Sources.size() || Mixed->Paths.size() != Sources.size() * (size_t)MMax)))
            throw std::runtime_error("FrequenSee: one row and MaxPaths paths per source");
        std::vector<fs_source> H;
        std::vector<fs_reflection_voice> All(Sources.size() * (size_t)Stride);
        std::vector<int32_t> N;
        for (size_t i = 0; i < Sources.size(); ++i) {
            H.push_back(Sources[i]->Handle_);
            const std::vector<fs_reflection_voice> V = Voices(Rows[i], Paths.data() + i * (size_t)MaxPaths, Right, ReferenceLength,
                                                              Diffraction ? &Diffraction->Rows[i] : nullptr,
                                                              Diffraction ? Diffraction->Paths.data() + i * (size_t)DMax : nullptr,
                                                              Second ? &Second->Rows[i] : nullptr,
                                                              Second ? Second->Paths.data() + i * (size_t)SMax : nullptr,
                                                              Thick ? &Thick->Rows[i] : nullptr,
                                                              Thick ? Thick->Paths.data() + i * (size_t)TMax : nullptr,
                                                              Mixed ? &Mixed->Rows[i] : nullptr,
                                                              Mixed ? Mixed->Paths.data() + i * (size_t)MMax : nullptr);
            std::copy(V.begin(), V.end(), All.begin() + (std::ptrdiff_t)(i * (size_t)Stride));
            N.push_back((int32_t)V.size());
        }
        SubSys_->Check(fs_reflection_render_process_batch(SubSys_->Ctx_, H.data(), (int32_t)H.size(), In, All.data(), N.data(), Stride, Out,
                                                          Mix, Counts));
    }

    int VoiceCount = FS_MAX_REFLECTION_VOICES;
};

// Not in the reference: the reflection plugin with every voice rendered from its arrival direction through a head-related impulse
// response set — fs_binaural_render_process_batch, one call for all sources — instead of a pan: interaural delay and head shadow
// come out of the set.  The direct sound becomes a voice of the same call.  The listener's orientation (Forward, Right) is the
// host's, and so is any measured HRIR set (SetHrtf); without one SetHrtf() installs the library's spherical-head model.
class FrequenSeeAudioBinauralPlugin : public FrequenSeeAudioReflectionPlugin {
public:
    explicit FrequenSeeAudioBinauralPlugin(AudioRayTracingSubsystem& SubSys) : FrequenSeeAudioReflectionPlugin(SubSys) {}
    // the context's set: Dirs [n][3] (head frame: x forward, y right, z up), Hrir [n][2][H].  Interpolate: triangulate the set and
    // install the mesh (fs_hrtf_set_mesh) — every voice's HRIR is then the blend of the three round its direction, not the nearest
    // one.  Align: carry the HRIRs' onsets apart (fs_hrtf_set_onsets), so that the blend is of aligned HRIRs and of their delays —
    // Onsets [n][2] where the host has them (Hrir is then the aligned set), else split off the set given (fs_hrtf_split_onsets:
    // threshold 0.1, lead 0).  Before OnInitSource; not concurrent with ProcessAudio
    void SetHrtf(const std::vector<float>& Dirs, const std::vector<float>& Hrir, int HrirTaps, bool Interpolate = false, bool Align = false,
                 const std::vector<float>* Onsets = nullptr) {
        if (HrirTaps < 1 || Dirs.size() % 3 != 0 || Hrir.size() != Dirs.size() / 3 * 2 * (size_t)HrirTaps ||
            (Onsets && (!Align || Onsets->size() != Dirs.size() / 3 * 2)))
            throw std::runtime_error("FrequenSee: an HRIR set is dirs [n][3], hrir [n][2][taps] and, with Align, onsets [n][2]");
        std::vector<float> Aligned, Split;
        if (Align && !Onsets) {
            Aligned.resize(Hrir.size());
            Split.resize(Dirs.size() / 3 * 2);
            if (fs_hrtf_split_onsets(Hrir.data(), (int32_t)(Dirs.size() / 3), HrirTaps, 0.1f, 0, Aligned.data(), Split.data()) != FS_OK)
                throw std::runtime_error("FrequenSee: fs_hrtf_split_onsets refused the set");
            Onsets = &Split;
        }
        fs_hrtf_desc D{};
        D.struct_size = sizeof(D);
        D.directions = (int32_t)(Dirs.size() / 3);
        D.taps = HrirTaps;
        D.sample_rate = SampleRate;
        D.dirs = Dirs.data();
        D.hrir = Aligned.empty() ? Hrir.data() : Aligned.data();
        SubSys_->Check(fs_hrtf_set(SubSys_->Ctx_, &D));
        if (Interpolate) {
            std::vector<int32_t> Tri((size_t)std::max(2 * D.directions - 4, 1) * 3);
            int32_t Triangles = 0;
            if (fs_hrtf_triangulate(Dirs.data(), D.directions, Tri.data(), (int32_t)(Tri.size() / 3), &Triangles) != FS_OK)
                throw std::runtime_error("FrequenSee: fs_hrtf_triangulate needs 4 .. 4096 distinct directions that surround the listener");
            SubSys_->Check(fs_hrtf_set_mesh(SubSys_->Ctx_, Tri.data(), Triangles));
        }
        if (Align) SubSys_->Check(fs_hrtf_set_onsets(SubSys_->Ctx_, Onsets->data()));
    }
    // ... or the spherical-head model (a model: interaural delay and level difference, no pinna); Align: its two halves apart
    void SetHrtf(int Directions = 1024, int HrirTaps = 128, bool Interpolate = false, bool Align = false) {
        std::vector<float> Dirs((size_t)std::max(Directions, 0) * 3), Hrir((size_t)std::max(Directions, 0) * 2 * (size_t)std::max(HrirTaps, 0));
        std::vector<float> Onsets((size_t)std::max(Directions, 0) * 2);
        const int Rc = Align ? fs_hrtf_spherical_head_split(SampleRate, FS_HRTF_DEFAULT_RADIUS_CM, FS_HRTF_DEFAULT_SOUND_SPEED_CM_S, Directions,
                                                            HrirTaps, Dirs.data(), Hrir.data(), Onsets.data())
                             : fs_hrtf_spherical_head(SampleRate, FS_HRTF_DEFAULT_RADIUS_CM, FS_HRTF_DEFAULT_SOUND_SPEED_CM_S, Directions, HrirTaps,
                                                      Dirs.data(), Hrir.data());
        if (Rc != FS_OK) throw std::runtime_error("FrequenSee: fs_hrtf_spherical_head refused the directions or the taps");
        SetHrtf(Dirs, Hrir, HrirTaps, Interpolate, Align, Align ? &Onsets : nullptr);
    }
    void OnInitSource(const FrequenSeeAudioComponent& C) {
        SubSys_->Check(fs_binaural_render_init(SubSys_->Ctx_, C.Handle_, FrameSize, Taps, VoiceCount, MaxDelaySeconds));
    }
    void OnReleaseSource(const FrequenSeeAudioComponent& C) { SubSys_->Check(fs_binaural_render_release(SubSys_->Ctx_, C.Handle_)); }
    // One source's entries: keys, delays and band gains exactly as FrequenSeeAudioReflectionPlugin::Voices builds them, from the same
    // arguments; gain = min(1, ReferenceLength / length) with ReferenceLength > 0 (cm), else 1; direction = the path's arrival
    // direction d in the head frame, (d . Forward, d . Right, d . Up) with Up = (F.Y R.Z - F.Z R.Y, F.Z R.X - F.X R.Z, F.X R.Y - F.Y R.X)
    // — for Forward = +x and Right = +y that is +z.  Direct (the source's row of fs_update_direct_paths) with ToSource (the vector from
    // the listener to the source, world space, any length but zero) puts the direct sound in front as one more voice: key =
    // FS_BINAURAL_DIRECT_KEY (a triangle index no scene of fewer than 2^29 - 1 triangles has: a first-order path with it is refused),
    // band_gain = transmission, length = distance
    std::vector<fs_binaural_voice> Voices(const fs_reflection_row& Row, const fs_reflection_path* Paths, const FVector& Forward, const FVector& Right,
                                          float ReferenceLength = 0.0f, const fs_direct_path* Direct = nullptr, const FVector* ToSource = nullptr,
                                          const fs_diffraction_row* DRow = nullptr, const fs_diffraction_path* DPaths = nullptr,
                                          const fs_reflection2_row* SRow = nullptr, const fs_reflection2_path* SPaths = nullptr,
                                          const fs_diffraction2_row* TRow = nullptr, const fs_diffraction2_path* TPaths = nullptr,
                                          const fs_mixed_row* MRow = nullptr, const fs_mixed_path* MPaths = nullptr) const {
        const double F[3] = {Forward.X, Forward.Y, Forward.Z}, R[3] = {Right.X, Right.Y, Right.Z};
        const double U[3] = {F[1] * R[2] - F[2] * R[1], F[2] * R[0] - F[0] * R[2], F[0] * R[1] - F[1] * R[0]};
        std::vector<fs_binaural_voice> V;
        auto Add = [&](uint32_t Key, float Delay, const float* Gain, const double* Dir, float Length) {
            fs_binaural_voice O{};
            O.key = Key;
            O.delay = TargetDelay(Delay);
            for (int b = 0; b < FS_MAX_BANDS; ++b) O.band_gain[b] = Gain[b];
            O.gain = ReferenceLength > 0.0f ? (float)std::min(1.0, (double)ReferenceLength / (double)Length) : 1.0f;
            O.direction[0] = (float)(Dir[0] * F[0] + Dir[1] * F[1] + Dir[2] * F[2]);
            O.direction[1] = (float)(Dir[0] * R[0] + Dir[1] * R[1] + Dir[2] * R[2]);
            O.direction[2] = (float)(Dir[0] * U[0] + Dir[1] * U[1] + Dir[2] * U[2]);
            V.push_back(O);
        };
        const bool WithDirect = Direct && ToSource;
        if (WithDirect) {
            const double D[3] = {ToSource->X, ToSource->Y, ToSource->Z};
            Add(FS_BINAURAL_DIRECT_KEY, Direct->delay, Direct->transmission, D, Direct->distance);
        }
        ForEachVoice(Row, Paths, DRow, DPaths, SRow, SPaths, TRow, TPaths, MRow, MPaths,
                     [&](uint32_t Key, float Delay, const float* Gain, const float* Dir, float Length) {
                         if (WithDirect && Key == FS_BINAURAL_DIRECT_KEY)
                             throw std::runtime_error("FrequenSee: triangle index 2^29 - 1: its key is the direct sound's");
                         const double D[3] = {Dir[0], Dir[1], Dir[2]};
                         Add(Key, Delay, Gain, D, Length);
                     });
        return V;
    }
    // In [count][FrameSize * 2] interleaved stereo (a mono source in both channels), row i for Sources[i] and Voices[i] (what Voices
    // returned for it: FS_MAX_REFLECTION_VOICES entries at most); Out [count][FrameSize * 2] or nullptr, Mix [FrameSize * 2] or
    // nullptr, Counts [count] or nullptr
    void ProcessAudio(const std::vector<FrequenSeeAudioComponent*>& Sources, const float* In, const std::vector<std::vector<fs_binaural_voice>>& Voices,
                      float* Out, float* Mix = nullptr, fs_binaural_render_row* Counts = nullptr) {
        PackVoices(Sources, Voices, [&](const std::vector<fs_source>& H, const std::vector<fs_binaural_voice>& All, const std::vector<int32_t>& N, size_t Stride) {
            SubSys_->Check(fs_binaural_render_process_batch(SubSys_->Ctx_, H.data(), (int32_t)H.size(), In, All.data(), N.data(), (int32_t)Stride,
                                                            Out, Mix, Counts));
        });
    }

protected:
    // the handles, the voice table [count][Stride] and the counts a voice-bank callback takes, handed to Call
    template <typename CallT>
    void PackVoices(const std::vector<FrequenSeeAudioComponent*>& Sources, const std::vector<std::vector<fs_binaural_voice>>& Voices, CallT&& Call) {
        if (Voices.size() != Sources.size()) throw std::runtime_error("FrequenSee: one voice list per source");
        size_t Stride = 1;
        for (const auto& V : Voices) Stride = std::max(Stride, V.size());
        if (Stride > FS_MAX_REFLECTION_VOICES)
            throw std::runtime_error("FrequenSee: " + std::to_string(Stride) + " voices for one source, more than FS_MAX_REFLECTION_VOICES");
        std::vector<fs_source> H;
        std::vector<fs_binaural_voice> All(Sources.size() * Stride);
        std::vector<int32_t> N;
        for (size_t i = 0; i < Sources.size(); ++i) {
            H.push_back(Sources[i]->Handle_);
            std::copy(Voices[i].begin(), Voices[i].end(), All.begin() + (std::ptrdiff_t)(i * Stride));
            N.push_back((int32_t)Voices[i].size());
        }
        Call(H, All, N, Stride);
    }
};

// Not in the reference: the binaural plugin's voices — the same entries, Voices() inherited unchanged — rendered into an ambisonic
// bus of (Order + 1)^2 channels, ACN order and SN3D normalisation (fs_ambisonic_render_process_batch, one call for all sources),
// instead of two ears: for loudspeakers, for an engine's soundfield submix, for a host's own binaural decoder.  No HRIR set is
// needed.  The bus is rendered in the head frame given to Voices(); rotating it later (a head tracker) and decoding it are the host's.
class FrequenSeeAudioAmbisonicPlugin : public FrequenSeeAudioBinauralPlugin {
public:
    explicit FrequenSeeAudioAmbisonicPlugin(AudioRayTracingSubsystem& SubSys) : FrequenSeeAudioBinauralPlugin(SubSys) {}
    int Order = 1;   // 0 .. FS_MAX_AMBISONIC_ORDER; before OnInitSource
    int Channels() const { return (Order + 1) * (Order + 1); }
    void OnInitSource(const FrequenSeeAudioComponent& C) {
        SubSys_->Check(fs_ambisonic_render_init(SubSys_->Ctx_, C.Handle_, FrameSize, Taps, VoiceCount, MaxDelaySeconds, Order));
    }
    void OnReleaseSource(const FrequenSeeAudioComponent& C) { SubSys_->Check(fs_ambisonic_render_release(SubSys_->Ctx_, C.Handle_)); }
    // In [count][FrameSize * 2] interleaved stereo (a mono source in both channels; the renderer takes their mean), row i for
    // Sources[i] and Voices[i]; Out [count][FrameSize][Channels()] or nullptr, Mix [FrameSize][Channels()] or nullptr, Counts
    // [count] or nullptr
    void ProcessAudio(const std::vector<FrequenSeeAudioComponent*>& Sources, const float* In, const std::vector<std::vector<fs_ambisonic_voice>>& Voices,
                      float* Out, float* Mix = nullptr, fs_ambisonic_render_row* Counts = nullptr) {
        PackVoices(Sources, Voices, [&](const std::vector<fs_source>& H, const std::vector<fs_ambisonic_voice>& All, const std::vector<int32_t>& N, size_t Stride) {
            SubSys_->Check(fs_ambisonic_render_process_batch(SubSys_->Ctx_, H.data(), (int32_t)H.size(), In, All.data(), N.data(), (int32_t)Stride,
                                                             Out, Mix, Counts));
        });
    }
};

}  // namespace frequensee
