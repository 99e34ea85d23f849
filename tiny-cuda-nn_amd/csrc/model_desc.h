// model_desc.h -- description of a model (encoding + optional fully fused network): what the JSON configuration asks for, resolved
// into the metadata the kernels take, plus parameter initialisation.  Mirrors the reference's
//   include/tiny-cuda-nn/config.h:46-63, network_with_input_encoding.h:55-130, grid.h:673-737/1725-1852, src/network.cu:51-138
// for the HashGrid + FullyFusedMLP hot path only.
#pragma once
#include <string>
#include <vector>

#include "../../include/tiny-cuda-nn/json_mini.h"
#include "adam_device.h"
#include "composite_kernels.h"
#include "elementwise_kernels.h"
#include "grid_kernels.h"
#include "mlp_kernels.h"

namespace tcnn_hip {

enum class EncodingKind : uint32_t { Identity = 0, OneBlob = 1, Frequency = 2, TriangleWave = 3, Grid = 4, Composite = 5 };
enum class ReductionType : uint32_t { Concatenation = 0, Sum = 1, Product = 2 };  // common.h ReductionType

struct EncodingDesc {
	EncodingKind kind = EncodingKind::Identity;
	// grid (grid.h:673-737)
	GridMeta grid = {};
	uint32_t log2_hashmap_size = 19, base_resolution = 16;
	float per_level_scale = 2.0f;
	// identity (identity.h:88-93)
	float id_scale = 1.0f, id_offset = 0.0f;
	// one-blob (oneblob.h:168-178): n_bins outputs per input dimension
	uint32_t n_bins = 0;
	// frequency (frequency.h:106-111): sin and cos of n_frequencies octaves per input dimension; triangle wave (triangle_wave.h:113-116):
	// one output per octave
	uint32_t n_frequencies = 0;
	uint32_t n_dims = 0;
	uint32_t n_output_dims = 0;  // before padding (a Composite's: its padded width, composite.h:374-376)
	uint32_t n_params = 0;
	uint32_t padded_output_width = 0;
	// composite (composite.h:138-212): the nested encodings in order.  Each one carries its own place in the composite: the first
	// input dimension it reads, the first row of the (unreduced) encoded matrix it writes -- n_dims and padded_output_width are its
	// input and padded output width -- and where its parameters start behind the composite's first one.
	ReductionType reduction = ReductionType::Concatenation;
	std::vector<EncodingDesc> nested;
	uint32_t dims_to_encode_begin = 0, output_row = 0, param_offset = 0;

	// the top-level encoding is a single grid: what level groups, the LDS budget, grid_level_* / grid_indices, second-order gradients
	// and the optimizer's per-level deficits apply to.  Grids nested in a Composite take the plain path.
	bool is_grid() const { return kind == EncodingKind::Grid; }
	// Run-time state of such a grid, as in the reference (multi_level_interface.h:101-123): not a hyperparameter, not serialized.  The scalar
	// lives in grid.max_level; the array is the CALLER'S device memory, one float per sample of every later call, and wins over the scalar.
	const float* max_level_gpu = nullptr;
	bool is_composite() const { return kind == EncodingKind::Composite; }
	bool has_nested_grid() const;
	uint32_t unreduced_width() const { return reduction == ReductionType::Concatenation ? padded_output_width : padded_output_width * (uint32_t)nested.size(); }
	uint32_t required_output_alignment() const;  // grid.h:1066-1068, composite.h:394-400
	void set_alignment(uint32_t alignment);  // encoding.h:70-72
	void set_padded_output_width(uint32_t width);  // composite.h:382-392
	const char* name() const;
	Json hyperparams() const;
};

struct NetworkDesc {
	MlpMeta mlp = {};
	uint32_t n_output_dims = 0;
	uint32_t n_hidden_layers = 0;
	std::string otype;
	// weights, activations and gradients are float and the network is the fp32 layer-by-layer one (mlp_kernels.h mlp_f32_*) under every `otype`
	// spelling: what the reference built without half precision makes of every network (network.cu:51-138 with network_precision_t = float)
	bool fp32 = false;
	Json hyperparams() const;  // fully_fused_mlp.h:139-147
};

// A NetworkWithInputEncoding (network_with_input_encoding.h:40-130) or a bare encoding.
struct Model {
	uint32_t n_input_dims = 0;
	EncodingDesc enc;
	bool has_network = false;
	NetworkDesc net;
	std::string hyper_json;

	size_t n_mlp_params() const { return has_network ? net.mlp.n_params() : 0; }
	size_t n_params() const { return n_mlp_params() + enc.n_params; }  // network first, then encoding (:115-122)
	uint32_t padded_output_width() const { return has_network ? net.mlp.padded_out : enc.padded_output_width; }
	uint32_t output_width() const { return has_network ? net.n_output_dims : enc.padded_output_width; }
	std::string name() const { return has_network ? "NetworkWithInputEncoding" : enc.name(); }

	// set_max_level / set_max_level_gpu apply where the top-level encoding is a single grid: why they do not apply here (empty: they do)
	std::string max_level_refusal() const {
		if (enc.is_grid()) return "";
		return std::string("set_max_level: ") + enc.name() + " is not a multi-level grid encoding" +
		       (enc.is_composite() ? " (grids nested in a CompositeEncoding take the plain path: max_level does not reach them)" : "");
	}

	void finish();  // fills hyper_json
	// network_with_input_encoding.h:124-130 + fully_fused_mlp.cu:868-893 + grid.h:1076-1079
	void initialize_params(hipStream_t stream, Pcg32& rng, float* params_full_precision, float scale) const;
};

EncodingDesc create_encoding_desc(uint32_t n_dims, const Json& enc, uint32_t alignment);  // encoding.cu:131-145
Model make_nwie(uint32_t n_input_dims, uint32_t n_output_dims, const Json& encoding, const Json& network, bool fp32_network = false);
const char* loss_name(LossType loss);  // loss.cu:57-65
LossType string_to_loss(const std::string& s);
void parse_adam(AdamHyper& h, const Json& p);  // adam.h:221-281

}  // namespace tcnn_hip
