// model_desc.hip -- JSON -> model description factories, enum <-> string tables, hyper-parameter JSON, parameter initialisation.
#include "model_desc.h"

#include <cmath>
#include <limits>
#include <vector>

#include "host_common.h"

namespace tcnn_hip {

// ------------------------------------------------------------------------------------------------
// model description
// ------------------------------------------------------------------------------------------------
static uint32_t powi(uint32_t base, uint32_t exponent) {
	uint32_t r = 1;
	for (uint32_t i = 0; i < exponent; ++i) r *= base;
	return r;
}

static const char* to_string(GridType t) { return t == GridType::Hash ? "Hash" : t == GridType::Dense ? "Dense" : "Tiled"; }
static const char* to_string(InterpolationType t) {
	return t == InterpolationType::Nearest ? "Nearest" : t == InterpolationType::Linear ? "Linear" : "Smoothstep";
}
static const char* const ACTIVATION_NAMES[] = {"None", "ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh", "SiLU", "Sine"};
static const char* to_string(Activation a) { return ACTIVATION_NAMES[(int)a]; }

static GridType string_to_grid_type(const std::string& s) {  // common_host.cu:112-122
	if (equals_case_insensitive(s, "Hash")) return GridType::Hash;
	if (equals_case_insensitive(s, "Dense")) return GridType::Dense;
	if (equals_case_insensitive(s, "Tiled") || equals_case_insensitive(s, "Tile")) return GridType::Tiled;
	throw std::runtime_error("Invalid grid type: " + s);
}
static InterpolationType string_to_interpolation_type(const std::string& s) {  // common_host.cu:160-170
	if (equals_case_insensitive(s, "Nearest")) return InterpolationType::Nearest;
	if (equals_case_insensitive(s, "Linear")) return InterpolationType::Linear;
	if (equals_case_insensitive(s, "Smoothstep")) return InterpolationType::Smoothstep;
	throw std::runtime_error("Invalid interpolation type: " + s);
}
static Activation string_to_activation(const std::string& s) {  // common_host.cu:70-96
	// (SiLU and Sine parse like the others; where they are allowed is create_network_desc's business)
	for (size_t i = 0; i < sizeof(ACTIVATION_NAMES) / sizeof(ACTIVATION_NAMES[0]); ++i) {
		if (equals_case_insensitive(s, ACTIVATION_NAMES[i])) return (Activation)i;
	}
	throw std::runtime_error("Invalid activation name: " + s);  // common_host.cu:94
}

static uint32_t lcm(uint32_t a, uint32_t b) {
	uint32_t x = a, y = b;
	while (y) {
		uint32_t t = x % y;
		x = y;
		y = t;
	}
	return a / x * b;
}

bool EncodingDesc::has_nested_grid() const {
	for (const EncodingDesc& e : nested) {
		if (e.is_grid()) return true;
	}
	return false;
}

uint32_t EncodingDesc::required_output_alignment() const {
	if (is_grid()) return grid.n_feat;  // grid.h:1066-1068
	uint32_t alignment = 1;
	for (const EncodingDesc& e : nested) alignment = lcm(alignment, e.required_output_alignment());  // composite.h:394-400
	return alignment;
}

void EncodingDesc::set_padded_output_width(uint32_t width) {
	if (!is_composite()) {
		if (width < n_output_dims) throw std::runtime_error(std::string(name()) + ": the padded output width " + std::to_string(width) + " is below the output width " + std::to_string(n_output_dims));
		padded_output_width = width;
		return;
	}
	if (nested.empty()) return;
	if (reduction == ReductionType::Concatenation) {  // composite.h:383-386: the last nested encoding takes the padding
		const uint32_t prev_n_dims = padded_output_width - nested.back().padded_output_width;
		if (width < prev_n_dims) throw std::runtime_error("CompositeEncoding: the padded output width is below the width of the leading nested encodings");
		nested.back().set_padded_output_width(width - prev_n_dims);
		padded_output_width = width;
	} else {  // composite.h:388-390
		for (uint32_t i = 0; i < nested.size(); ++i) {
			nested[i].set_padded_output_width(width);
			nested[i].output_row = i * width;
		}
		padded_output_width = width;
	}
	n_output_dims = padded_output_width;  // composite.h:374-376
}

void EncodingDesc::set_alignment(uint32_t alignment) {
	const uint32_t l = lcm(alignment, required_output_alignment());
	if (is_composite()) {
		set_padded_output_width(next_multiple(padded_output_width, l));
	} else {
		padded_output_width = next_multiple(n_output_dims, l);
	}
}

const char* EncodingDesc::name() const {
	switch (kind) {
		case EncodingKind::Grid: return "GridEncoding";
		case EncodingKind::OneBlob: return "OneBlobEncoding";
		case EncodingKind::Frequency: return "FrequencyEncoding";
		case EncodingKind::TriangleWave: return "TriangleWaveEncoding";
		case EncodingKind::Composite: return "CompositeEncoding";
		default: return "IdentityEncoding";
	}
}

Json EncodingDesc::hyperparams() const {
	Json j = Json::object();
	if (is_grid()) {  // grid.h:1115-1132
		j["otype"] = "Grid";
		j["type"] = to_string((GridType)grid.grid_type);
		j["n_levels"] = grid.n_levels;
		j["n_features_per_level"] = grid.n_feat;
		j["base_resolution"] = base_resolution;
		j["per_level_scale"] = per_level_scale;
		j["interpolation"] = to_string((InterpolationType)grid.interp);
		j["hash"] = "CoherentPrime";
		if ((GridType)grid.grid_type == GridType::Hash) j["log2_hashmap_size"] = log2_hashmap_size;
	} else if (kind == EncodingKind::Frequency) {  // frequency.h:200-205
		j["otype"] = "Frequency";
		j["n_frequencies"] = n_frequencies;
	} else if (kind == EncodingKind::TriangleWave) {  // triangle_wave.h:205-210
		j["otype"] = "TriangleWave";
		j["n_frequencies"] = n_frequencies;
	} else if (kind == EncodingKind::OneBlob) {  // oneblob.h:296-301
		j["otype"] = "OneBlob";
		j["n_bins"] = n_bins;
	} else if (is_composite()) {  // composite.h:439-449 (no "reduction" key, as there)
		Json list = Json::array();
		for (const EncodingDesc& e : nested) list.push_back(e.hyperparams());
		j["otype"] = "Composite";
		j["nested"] = list;
	} else {
		j["otype"] = "Identity";
		j["scale"] = id_scale;
		j["offset"] = id_offset;
	}
	return j;
}

static EncodingDesc create_grid_encoding(uint32_t n_dims, const Json& enc) {  // grid.h:1725-1852
	EncodingDesc e;
	e.kind = EncodingKind::Grid;
	e.n_dims = n_dims;
	const std::string hash = enc.value("hash", "CoherentPrime");
	if (!equals_case_insensitive(hash, "CoherentPrime")) throw std::runtime_error("GridEncoding: compiled without " + hash + " hash support.");
	const uint32_t F = enc.value("n_features_per_level", 2u);
	if (F != 1 && F != 2 && F != 4 && F != 8) throw std::runtime_error("GridEncoding: n_features_per_level must be 1, 2, 4, or 8.");
	const uint32_t log2_hashmap_size = enc.value("log2_hashmap_size", 19u);
	const std::string otype = enc.value("otype", "Grid");
	const std::string default_type = equals_case_insensitive(otype, "TiledGrid") ? "Tiled" : (equals_case_insensitive(otype, "DenseGrid") ? "Dense" : "Hash");
	uint32_t n_features;
	if (enc.contains("n_features") || enc.contains("n_grid_features")) {
		n_features = (uint32_t)(enc.contains("n_features") ? enc["n_features"] : enc["n_grid_features"]).as_number();
		if (enc.contains("n_levels")) throw std::runtime_error("GridEncoding: may not specify n_features and n_levels simultaneously (one determines the other)");
	} else {
		n_features = F * enc.value("n_levels", 16u);
	}
	const uint32_t n_levels = n_features / F;
	const GridType grid_type = string_to_grid_type(enc.value("type", default_type));
	const uint32_t base_resolution = enc.value("base_resolution", 16u);
	const float default_scale = grid_type == GridType::Dense ? std::exp(std::log(256.0f / (float)base_resolution) / (float)(n_levels - 1)) : 2.0f;
	const float per_level_scale = enc.value("per_level_scale", default_scale);

	const InterpolationType interp = string_to_interpolation_type(enc.value("interpolation", "Linear"));
	if (n_dims < 2 || n_dims > 4) throw std::runtime_error("GridEncoding: number of input dims must be 2, 3 or 4.");
	if (n_levels > MAX_N_LEVELS) throw std::runtime_error("GridEncoding: m_n_levels=" + std::to_string(n_levels) + " must be at most MAX_N_LEVELS=" + std::to_string(MAX_N_LEVELS));
	if (n_features % F != 0) throw std::runtime_error("GridEncoding: n_features=" + std::to_string(n_features) + " must be a multiple of N_FEATURES_PER_LEVEL=" + std::to_string(F));

	GridMeta& g = e.grid;
	g.n_dims = n_dims;
	g.n_levels = n_levels;
	g.n_feat = F;
	g.grid_type = (uint32_t)grid_type;
	g.interp = (uint32_t)interp;
	g.max_level = 1.0f;
	g.stochastic = enc.value("stochastic_interpolation", false) ? 1u : 0u;  // grid.h:1752
	// grid.h:699-727; the scale / resolution table is computed here once (fp32, same expressions as
	// common_device.h:886-895) and handed to the kernels, see GridMeta.
	const float log2_per_level_scale = std::log2(per_level_scale);
	uint32_t offset = 0;
	for (uint32_t i = 0; i < n_levels; ++i) {
		const float scale = exp2f((float)i * log2_per_level_scale) * (float)base_resolution - 1.0f;
		const uint32_t resolution = (uint32_t)ceilf(scale) + 1;
		g.scale[i] = scale;
		g.resolution[i] = resolution;
		const uint32_t max_params = std::numeric_limits<uint32_t>::max() / 2;
		uint32_t params_in_level = std::pow((float)resolution, (float)n_dims) > (float)max_params ? max_params : powi(resolution, n_dims);
		params_in_level = next_multiple(params_in_level, 8u);
		if (grid_type == GridType::Tiled) {
			params_in_level = std::min(params_in_level, powi(base_resolution, n_dims));
		} else if (grid_type == GridType::Hash) {
			params_in_level = std::min(params_in_level, 1u << log2_hashmap_size);
		}
		g.offset[i] = offset;
		offset += params_in_level;
		log_message(TCNN_LOG_DEBUG, "GridEncoding at level " + std::to_string(i) + ": resolution=" + std::to_string(resolution) +
		                                " params_in_level=" + std::to_string(params_in_level));
	}
	g.offset[n_levels] = offset;
	e.n_params = offset * F;
	e.n_output_dims = n_features;
	e.padded_output_width = n_features;
	e.log2_hashmap_size = log2_hashmap_size;
	e.base_resolution = base_resolution;
	e.per_level_scale = per_level_scale;
	return e;
}

static ReductionType string_to_reduction_type(const std::string& s) {  // common_host.cu:220-232
	if (equals_case_insensitive(s, "Concatenation")) return ReductionType::Concatenation;
	if (equals_case_insensitive(s, "Sum")) return ReductionType::Sum;
	if (equals_case_insensitive(s, "Product")) return ReductionType::Product;
	throw std::runtime_error("Invalid reduction type: " + s);
}

static EncodingDesc create_composite_encoding(uint32_t n_dims, const Json& params) {  // composite.h:138-212
	if (!params.contains("nested") || !params["nested"].is_array()) {
		throw std::runtime_error("Must provide an array of nested encodings to CompositeEncoding.");
	}
	EncodingDesc c;
	c.kind = EncodingKind::Composite;
	c.n_dims = n_dims;
	c.reduction = string_to_reduction_type(params.value("reduction", "Concatenation"));
	const Json& nested = params["nested"];

	uint32_t total_nested_dims_to_encode = 0;
	for (size_t i = 0; i < nested.size(); ++i) {
		total_nested_dims_to_encode += nested[i].value("n_dims_to_encode", 0u);
		if (nested[i].contains("dims_to_encode_begin")) {
			total_nested_dims_to_encode = 0xFFFFFFFFu;
			break;
		}
	}
	if (total_nested_dims_to_encode != 0xFFFFFFFFu && total_nested_dims_to_encode > n_dims) {
		throw std::runtime_error("CompositeEncoding: nested encodings must not encode more dims " + std::to_string(total_nested_dims_to_encode) + " than composite " +
		                         std::to_string(n_dims));
	}
	uint32_t unspecified_dims_to_encode = total_nested_dims_to_encode == 0xFFFFFFFFu ? 0xFFFFFFFFu : (n_dims - total_nested_dims_to_encode);
	uint32_t offset = 0;
	for (size_t i = 0; i < nested.size(); ++i) {
		uint32_t nested_dims_to_encode;
		if (nested[i].contains("n_dims_to_encode")) {
			if (nested[i].contains("dims_to_encode_begin")) offset = (uint32_t)nested[i]["dims_to_encode_begin"].as_number();
			nested_dims_to_encode = (uint32_t)nested[i]["n_dims_to_encode"].as_number();
		} else {
			if (unspecified_dims_to_encode == 0xFFFFFFFFu) {
				throw std::runtime_error("CompositeEncoding: may only leave 'n_dims_to_encode' unspecified for a single nested encoding");
			}
			nested_dims_to_encode = unspecified_dims_to_encode;
			unspecified_dims_to_encode = 0xFFFFFFFFu;
		}
		if (nested_dims_to_encode > 0) {
			const std::string otype = nested[i].value("otype", "OneBlob");
			if (equals_case_insensitive(otype, "Composite") || equals_case_insensitive(otype, "NRC") || equals_case_insensitive(otype, "OneBlobFrequency")) {
				throw std::runtime_error("CompositeEncoding: a nested Composite encoding is not supported by this build (flatten the nested list)");
			}
			if ((uint64_t)offset + nested_dims_to_encode > n_dims) {
				throw std::runtime_error("CompositeEncoding: nested encoding " + std::to_string(i) + " reads dims [" + std::to_string(offset) + ", " +
				                         std::to_string((uint64_t)offset + nested_dims_to_encode) + ") of a composite with " + std::to_string(n_dims) + " dims");
			}
			EncodingDesc e = create_encoding_desc(nested_dims_to_encode, nested[i], 1);
			e.dims_to_encode_begin = offset;
			c.nested.push_back(e);
		}
		offset += nested_dims_to_encode;
	}
	// the reference lets a later nested encoding overwrite the dL_dinput rows of an earlier one that reads the same dims; refused here
	for (size_t i = 0; i < c.nested.size(); ++i) {
		for (size_t j = 0; j < i; ++j) {
			const EncodingDesc &a = c.nested[j], &b = c.nested[i];
			if (a.dims_to_encode_begin < b.dims_to_encode_begin + b.n_dims && b.dims_to_encode_begin < a.dims_to_encode_begin + a.n_dims) {
				throw std::runtime_error("CompositeEncoding: nested encodings " + std::to_string(j) + " and " + std::to_string(i) +
				                         " read overlapping input dims (dims_to_encode_begin); overlapping ranges are not supported by this build");
			}
		}
	}
	uint32_t n_parameterless = 0;
	for (const EncodingDesc& e : c.nested) n_parameterless += e.is_grid() ? 0u : 1u;
	if (n_parameterless > ENCODING_MAX_PARTS) {  // they run as ONE launch driven by a table that travels in the kernel arguments
		throw std::runtime_error("CompositeEncoding: more than " + std::to_string(ENCODING_MAX_PARTS) + " nested encodings without parameters are not supported by this build");
	}
	uint32_t param_offset = 0;
	for (EncodingDesc& e : c.nested) {  // composite.h:416-422
		e.param_offset = param_offset;
		param_offset += e.n_params;
	}
	c.n_params = param_offset;
	// composite.h:188-211: every nested output starts at a multiple of its required alignment
	if (c.reduction == ReductionType::Concatenation) {
		uint32_t dims_encoded_so_far = 0;
		for (size_t i = 0; i < c.nested.size(); ++i) {
			EncodingDesc& e = c.nested[i];
			if (i + 1 < c.nested.size()) {
				const uint32_t desired_alignment = c.nested[i + 1].required_output_alignment();
				e.set_padded_output_width(next_multiple(dims_encoded_so_far + e.padded_output_width, desired_alignment) - dims_encoded_so_far);
			}
			e.output_row = dims_encoded_so_far;
			dims_encoded_so_far += e.padded_output_width;
		}
		c.padded_output_width = dims_encoded_so_far;
	} else {
		const uint32_t alignment = c.required_output_alignment();
		for (EncodingDesc& e : c.nested) e.set_alignment(alignment);
		for (size_t i = 0; i < c.nested.size(); ++i) {
			if (c.nested[i].padded_output_width != c.nested[0].padded_output_width) {
				throw std::runtime_error("CompositeEncoding: a Sum / Product reduction needs nested encodings of equal output width, but nested 0 has " +
				                         std::to_string(c.nested[0].padded_output_width) + " and nested " + std::to_string(i) + " has " + std::to_string(c.nested[i].padded_output_width));
			}
			c.nested[i].output_row = (uint32_t)i * c.nested[0].padded_output_width;
		}
		c.padded_output_width = c.nested.empty() ? 0u : c.nested[0].padded_output_width;
	}
	c.n_output_dims = c.padded_output_width;  // composite.h:374-376
	return c;
}

EncodingDesc create_encoding_desc(uint32_t n_dims, const Json& enc, uint32_t alignment) {  // encoding.cu:131-145
	const std::string name = enc.value("otype", "OneBlob");
	EncodingDesc e;
	if (equals_case_insensitive(name, "Grid") || equals_case_insensitive(name, "HashGrid") || equals_case_insensitive(name, "DenseGrid") ||
	    equals_case_insensitive(name, "TiledGrid")) {
		e = create_grid_encoding(n_dims, enc);
	} else if (equals_case_insensitive(name, "Composite")) {
		e = create_composite_encoding(n_dims, enc);
	} else if (equals_case_insensitive(name, "NRC") || equals_case_insensitive(name, "OneBlobFrequency")) {  // encoding.cu:93-115
		Json tri = Json::object(), blob = Json::object(), rest = Json::object();
		tri["n_dims_to_encode"] = 3u;
		tri["otype"] = "TriangleWave";
		tri["n_frequencies"] = enc.value("n_frequencies", 12u);
		blob["n_dims_to_encode"] = 5u;
		blob["otype"] = "OneBlob";
		blob["n_bins"] = enc.value("n_bins", 4u);
		rest["otype"] = "Identity";
		Json list = Json::array();
		list.push_back(tri);
		list.push_back(blob);
		list.push_back(rest);
		Json composite = Json::object();
		composite["otype"] = "Composite";
		composite["nested"] = list;
		e = create_composite_encoding(n_dims, composite);
	} else if (equals_case_insensitive(name, "Identity")) {
		e.kind = EncodingKind::Identity;
		e.n_dims = n_dims;
		e.id_scale = enc.value("scale", 1.0f);
		e.id_offset = enc.value("offset", 0.0f);
		e.n_output_dims = n_dims;
		e.padded_output_width = n_dims;
	} else if (equals_case_insensitive(name, "Frequency")) {  // encoding.cu:65-67
		e.kind = EncodingKind::Frequency;
		e.n_dims = n_dims;
		e.n_frequencies = enc.value("n_frequencies", 12u);
		if (e.n_frequencies == 0 || e.n_frequencies > 32) throw std::runtime_error("FrequencyEncoding: n_frequencies must be in [1, 32]");
		e.n_output_dims = n_dims * e.n_frequencies * 2u;
		e.padded_output_width = e.n_output_dims;
	} else if (equals_case_insensitive(name, "TriangleWave")) {  // encoding.cu:89-91
		e.kind = EncodingKind::TriangleWave;
		e.n_dims = n_dims;
		e.n_frequencies = enc.value("n_frequencies", 12u);
		if (e.n_frequencies == 0 || e.n_frequencies > 32) throw std::runtime_error("TriangleWaveEncoding: n_frequencies must be in [1, 32]");
		e.n_output_dims = n_dims * e.n_frequencies;
		e.padded_output_width = e.n_output_dims;
	} else if (equals_case_insensitive(name, "OneBlob")) {  // encoding.cu:118-120
		e.kind = EncodingKind::OneBlob;
		e.n_dims = n_dims;
		e.n_bins = enc.value("n_bins", 16u);
		if (e.n_bins == 0 || (e.n_bins & (e.n_bins - 1)) != 0) throw std::runtime_error("Number of bins must be a power of 2");  // oneblob.h:174-176
		e.n_output_dims = n_dims * e.n_bins;
		e.padded_output_width = e.n_output_dims;
	} else {
		throw std::runtime_error("Encoding '" + name + "' not found (this build provides Grid/HashGrid/DenseGrid/TiledGrid, Frequency, TriangleWave, OneBlob, Identity, "
		                         "Composite and its shortcuts NRC/OneBlobFrequency)");
	}
	if (alignment > 0) e.set_alignment(alignment);
	return e;
}

Json NetworkDesc::hyperparams() const {
	Json j = Json::object();
	j["otype"] = fp32 || mlp_layer_by_layer(mlp) ? "CutlassMLP" : "FullyFusedMLP";  // cutlass_mlp.h:152, fully_fused_mlp.h:141
	j["activation"] = to_string((Activation)mlp.activation);
	j["output_activation"] = to_string((Activation)mlp.output_activation);
	j["n_neurons"] = mlp.width;
	j["n_hidden_layers"] = n_hidden_layers;
	return j;
}

// fp32: the fp32 layer-by-layer network whatever the spelling (the reference without half precision: every network is a CutlassMLP) -- no
// fused width is special, the limits and their texts are the layer-by-layer network's
static NetworkDesc create_network_desc(uint32_t n_input_dims, uint32_t n_output_dims, const Json& net, bool fp32) {  // network.cu:51-138
	const std::string otype = net.value("otype", "MLP");
	const bool known = equals_case_insensitive(otype, "MegakernelMLP") || equals_case_insensitive(otype, "FullyFusedMLP") ||
	                   equals_case_insensitive(otype, "MLP") || equals_case_insensitive(otype, "CutlassMLP");
	if (!known) throw std::runtime_error("Invalid network type: " + otype);
	NetworkDesc d;
	d.otype = otype;
	d.fp32 = fp32;
	const uint32_t n_neurons = net.value("n_neurons", 128u);
	// network.cu:51-77, 129-137: FullyFusedMLP exists for four widths; "MLP" / "CutlassMLP" take those where they can and the
	// layer-by-layer network (mlp_general.hip) for every other multiple of 16
	const bool fused_width = !fp32 && mlp_fused_width(n_neurons);
	const bool wants_fused = !fp32 && (equals_case_insensitive(otype, "MegakernelMLP") || equals_case_insensitive(otype, "FullyFusedMLP"));
	if (!fused_width && wants_fused) {
		throw std::runtime_error("FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got " + std::to_string(n_neurons) +
		                         ". Use CutlassMLP instead.");
	}
	if (!fused_width && n_neurons % 16 != 0) {
		throw std::runtime_error("CutlassMLP: the number of neurons must be a multiple of 16, but got " + std::to_string(n_neurons) + ".");
	}
	if (!fused_width && (n_neurons < 16 || n_neurons > MLP_GENERAL_MAX_WIDTH)) {
		throw std::runtime_error("CutlassMLP: between 16 and " + std::to_string(MLP_GENERAL_MAX_WIDTH) + " neurons are supported by this build, but got " + std::to_string(n_neurons) + ".");
	}
	// SiLU and Sine need stored pre-activations, which FullyFusedMLP does not keep (common_device.h:377-386): as hidden activations they
	// make a network of ANY width a layer-by-layer one (cutlass_mlp.cu:53: no fused activation epilogue either); as output activations
	// nobody's backward pass has them (common_device.h:375-390 is an empty case) -- refused instead of a silently missing derivative
	const std::string act_name = net.value("activation", "ReLU"), out_act_name = net.value("output_activation", "None");
	const Activation act = string_to_activation(act_name);
	const Activation out_act = string_to_activation(out_act_name);
	if (act_needs_preactivation((uint32_t)act) && wants_fused) {
		throw std::runtime_error("Activation '" + act_name + "' is not supported by FullyFusedMLP (it needs stored pre-activations); use CutlassMLP.");
	}
	if (act_needs_preactivation((uint32_t)out_act)) {
		throw std::runtime_error("Activation '" + out_act_name + "' is not supported as output_activation: output activations must be expressible from the output value "
		                         "(the backward pass takes their derivative at the stored output; this one needs the pre-activation).");
	}
	// more than MLP_MAX_OUT_WIDTH (padded) outputs: layer by layer as well, under either spelling -- the reference's FullyFusedMLP hands a
	// last layer of more than 16 outputs to a plain matrix product (fully_fused_mlp.cu:786), its CutlassMLP takes any width
	d.mlp.width = n_neurons;
	d.mlp.activation = (uint32_t)act;
	d.mlp.padded_out = next_multiple(n_output_dims, 16u);  // fully_fused_mlp.cu:656
	const bool fused = !fp32 && !mlp_layer_by_layer(d.mlp);
	const char* const name = fused ? "FullyFusedMLP" : "CutlassMLP";
	d.n_hidden_layers = net.value("n_hidden_layers", 5u);
	if (d.n_hidden_layers == 0) throw std::runtime_error(std::string(name) + " requires at least 1 hidden layer (3 layers in total).");
	d.n_output_dims = n_output_dims;
	d.mlp.in_width = n_input_dims;
	d.mlp.n_hidden_matmuls = d.n_hidden_layers - 1;
	d.mlp.output_activation = (uint32_t)out_act;
	if (d.mlp.padded_out > MLP_GENERAL_MAX_OUT_WIDTH) {
		throw std::runtime_error(std::string(name) + ": more than " + std::to_string(MLP_GENERAL_MAX_OUT_WIDTH) + " output dimensions are not supported by this build.");
	}
	const uint32_t max_in = fused ? MLP_MAX_IN_WIDTH : MLP_GENERAL_MAX_IN_WIDTH;
	if (n_input_dims % 16 != 0 || n_input_dims > max_in) {
		throw std::runtime_error(std::string(name) + ": input width " + std::to_string(n_input_dims) + " must be a multiple of 16 and at most " + std::to_string(max_in));
	}
	return d;
}

void Model::finish() {
	Json j = Json::object();
	if (has_network) {
		j["otype"] = "NetworkWithInputEncoding";
		j["encoding"] = enc.hyperparams();
		j["network"] = net.hyperparams();
		hyper_json = j.dump();
	} else {
		hyper_json = enc.hyperparams().dump();
	}
}

void Model::initialize_params(hipStream_t stream, Pcg32& rng, float* params_full_precision, float scale) const {
	if (has_network) {
		std::vector<float> host(n_mlp_params());
		float* p = host.data();
		// uniform in [-s, s): next_float() * 2 * s - s, every step rounded to fp32 on its own (separate statements: no contraction)
		auto uniform = [&](uint32_t rows, uint32_t cols, float s) {
			for (size_t i = 0; i < (size_t)rows * cols; ++i) {
				float t = rng.next_float() * 2.0f;
				t = t * s;
				p[i] = t - s;
			}
			p += (size_t)rows * cols;
		};
		auto xavier = [&](uint32_t rows, uint32_t cols) { uniform(rows, cols, scale * std::sqrt(6.0f / (float)(rows + cols))); };  // gpu_matrix.h:292-307
		// SIREN (gpu_matrix.h:343-377, cutlass_mlp.cu:362-371): the first matrix 30 / fan_in, every other one sqrt(6 / fan_in); same rng, same order
		auto siren_first = [&](uint32_t rows, uint32_t cols) {
			const float f = 30.0f / (float)cols;
			uniform(rows, cols, scale * f);
		};
		auto siren = [&](uint32_t rows, uint32_t cols) {
			const float f = std::sqrt(6.0f / (float)cols);
			uniform(rows, cols, scale * f);
		};
		if (net.mlp.activation == (uint32_t)Activation::Sine) {
			siren_first(net.mlp.width, net.mlp.in_width);
			for (uint32_t i = 0; i < net.mlp.n_hidden_matmuls; ++i) siren(net.mlp.width, net.mlp.width);
			siren(net.mlp.padded_out, net.mlp.width);
		} else {
			xavier(net.mlp.width, net.mlp.in_width);
			for (uint32_t i = 0; i < net.mlp.n_hidden_matmuls; ++i) xavier(net.mlp.width, net.mlp.width);
			xavier(net.mlp.padded_out, net.mlp.width);
		}
		HIP_CHECK(hipMemcpyAsync(params_full_precision, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, stream));
		HIP_CHECK(hipStreamSynchronize(stream));
	}
	if (enc.is_composite()) {  // composite.h:424-429: the nested encodings in order, one rng
		for (const EncodingDesc& e : enc.nested) {
			if (e.n_params > 0) generate_random_uniform(stream, rng, e.n_params, params_full_precision + n_mlp_params() + e.param_offset, -1e-4f * scale, 1e-4f * scale);
		}
	} else if (enc.n_params > 0) {
		generate_random_uniform(stream, rng, enc.n_params, params_full_precision + n_mlp_params(), -1e-4f * scale, 1e-4f * scale);
	}
}

Model make_nwie(uint32_t n_input_dims, uint32_t n_output_dims, const Json& encoding, const Json& network, bool fp32_network) {
	Model md;
	md.n_input_dims = n_input_dims;
	md.enc = create_encoding_desc(n_input_dims, encoding, /*minimum_alignment(network)=*/16);  // network.cu:79-98 -> 16
	md.has_network = true;
	md.net = create_network_desc(md.enc.padded_output_width, n_output_dims, network, fp32_network);
	md.finish();
	return md;
}

static const char* const LOSS_NAMES[N_LOSS_TYPES] = {"L2",   "RelativeL2",   "L1",       "RelativeL1",         "Mape",
                                                    "Smape", "CrossEntropy", "Variance", "RelativeL2Luminance"};  // loss.cu:57-65
const char* loss_name(LossType loss) { return LOSS_NAMES[(int)loss]; }
LossType string_to_loss(const std::string& s) {
	for (int i = 0; i < N_LOSS_TYPES; ++i) {
		if (equals_case_insensitive(s, LOSS_NAMES[i])) return (LossType)i;
	}
	throw std::runtime_error("Loss '" + s + "' not found");  // loss.cu:86
}

void parse_adam(AdamHyper& h, const Json& p) {
	h.beta1 = p.value("beta1", h.beta1);
	h.beta2 = p.value("beta2", h.beta2);
	h.epsilon = p.value("epsilon", h.epsilon);
	h.learning_rate = p.value("learning_rate", h.learning_rate);
	h.l2_reg = p.value("l2_reg", h.l2_reg);
	h.adabound = p.value("adabound", h.adabound);
	h.relative_weight_decay = p.value("relative_decay", h.relative_weight_decay);
	h.absolute_weight_decay = p.value("absolute_decay", h.absolute_weight_decay);
	h.weight_clipping_magnitude = p.value("clipping_magnitude", h.weight_clipping_magnitude);
	h.gradient_clipping_magnitude = p.value("gradient_clipping_magnitude", h.gradient_clipping_magnitude);
	h.non_matrix_learning_rate_factor = p.value("non_matrix_learning_rate_factor", h.non_matrix_learning_rate_factor);
	h.non_matrix_l2_reg = p.value("non_matrix_l2_reg", h.non_matrix_l2_reg);
	h.optimize_matrix_params = p.value("optimize_matrix_params", h.optimize_matrix_params);
	h.optimize_non_matrix_params = p.value("optimize_non_matrix_params", h.optimize_non_matrix_params);
	h.skip_zero_grad_non_matrix_params = p.value("skip_zero_grad_non_matrix_params", h.skip_zero_grad_non_matrix_params);
}

}  // namespace tcnn_hip
