// Denoiser.h -- monoscale Bayesian collaborative denoiser, MI355X build.
// Public surface of the reference's include/bcd/core/Denoiser.h:25-44; the per-thread accumulator getters
// that only DenoisingUnit used (:36-44) do not exist here: the whole loop runs on the device behind
// include/bcd_hip.h.
#ifndef DENOISER_H
#define DENOISER_H

#include "IDenoiser.h"
#include "DeepImage.h"

#include <cstdint>
#include <vector>

namespace bcd
{

	/// Settings of this build that the reference's API has no place for.  Both denoiser classes expose them through the same
	/// setters; defaults reproduce the reference's behaviour on device 0.
	class HipEngineSettings
	{
	public:
		HipEngineSettings() : m_orderSeed(1234u), m_devices(1, 0), m_prefilterThresholdStDevFactor(0.f), m_zeroBadOutputValues(false), m_prefilterLayers(false), m_prefilterFrames(false), m_momentSelection(false), m_momentVarianceFloor(1e-8f),
				m_pGuideFeatures(nullptr), m_pGuideVariances(nullptr), m_guideThreshold(1.f) {}

		/// seed of the visiting order of -r 1 (the reference seeds its shuffle from the wall clock, src/core/Denoiser.cpp:418)
		void setOrderSeed(uint32_t i_seed) { m_orderSeed = i_seed; }
		/// HIP device; several devices split the frame into row bands (bcd_hip_multi_*, RCCL over xGMI between neighbours)
		void setDevice(int i_device) { m_devices.assign(1, i_device); }
		void setDevices(const std::vector<int>& i_rDevices) { if(!i_rDevices.empty()) m_devices = i_rDevices; }
		const std::vector<int>& getDevices() const { return m_devices; }
		/// > 0: run SpikeRemovalFilter::filter on the uploaded copies of the inputs before denoising (what bcd_cli -p 1 does on
		/// the host, src/cli/main.cpp:428-441); the caller's images are not modified.  One device only.
		void setSpikePrefilter(float i_thresholdStDevFactor) { m_prefilterThresholdStDevFactor = i_thresholdStDevFactor; }
		/// put negative / infinite / NaN output values to zero on the device (src/cli/main.cpp:389-420)
		void setZeroBadOutputValues(bool i_enabled) { m_zeroBadOutputValues = i_enabled; }

		/// A further colour layer (light group, diffuse / specular / ... pass) denoised WITH THE FILTER OF THE PRIMARY INPUTS: same similar
		/// patches, same processed pixels, one selection for all layers (bcd_hip_denoise_layers).  The DenoiserInputs colour and covariance
		/// images are layer 0; every added layer brings its own mean colours (W x H x 3) and sample covariances (W x H x 6) and shares the
		/// sample counts and histograms.  Non-owning pointers, like DenoiserInputs; the output is resized and overwritten.  At most
		/// 15 added layers, one device, and the spike prefilter only with setSpikePrefilterLayers(true).  With no added layer denoise() is
		/// what it always was.
		struct ColorLayer
		{
			const DeepImage<float>* m_pColors;
			const DeepImage<float>* m_pSampleCovariances;
			DeepImage<float>* m_pDenoisedColors;
		};
		void addLayer(const DeepImage<float>* i_pColors, const DeepImage<float>* i_pSampleCovariances, DeepImage<float>* o_pDenoisedColors)
		{
			ColorLayer layer = { i_pColors, i_pSampleCovariances, o_pDenoisedColors };
			m_layers.push_back(layer);
		}
		void clearLayers() { m_layers.clear(); }
		const std::vector<ColorLayer>& getLayers() const { return m_layers; }
		void setLayers(const std::vector<ColorLayer>& i_rLayers) { m_layers = i_rLayers; }
		/// true: a spike prefilter beside added colour layers is accepted and covers EVERY layer -- the filter decides from the primary
		/// colours which neighbour replaces a pixel, and each layer's colours and covariances are gathered through that decision on the
		/// device (bcd_hip_denoise_layers_host_ex).  false (default): the combination is refused, as it always was.
		void setSpikePrefilterLayers(bool i_enabled) { m_prefilterLayers = i_enabled; }
		bool getSpikePrefilterLayers() const { return m_prefilterLayers; }
		/// true: a spike prefilter beside neighbour frames (addNeighbourFrame, addNeighbourFrameMoments) and in a SequenceDenoiser is accepted: EVERY frame is
		/// prefiltered on its own -- its sample counts, its histograms and all its layers gathered through the decision taken on its own primary colours, in its
		/// own pixel grid (before a motion field reprojects it); feature buffers are not moved (bcd_hip_denoise_temporal_host_ex,
		/// bcd_hip_sequence_set_prefilter).  Beside neighbour frames the switch covers every layer of every frame and setSpikePrefilterLayers is not consulted.
		/// Without neighbour frames it changes nothing.  false (default): the combinations are refused, as they always were.
		void setSpikePrefilterFrames(bool i_enabled) { m_prefilterFrames = i_enabled; }
		bool getSpikePrefilterFrames() const { return m_prefilterFrames; }
		/// true: similar patches are selected from the primary colours and sample covariances (bcd_hip_denoise_moments_host) and NO histogram image is
		/// required -- DenoiserInputs::m_pHistograms may stay null.  m_histogramDistanceThreshold then thresholds the variance-normalised squared
		/// difference of the pixel means (expectation 1 between pixels of equal signal), not the chi-square histogram distance.  i_varFloor (finite, >= 0)
		/// is added to every summed variance.  Added layers and the prefilter switches work as with histograms; one device only.
		void setMomentSelection(bool i_enabled, float i_varFloor = 1e-8f) { m_momentSelection = i_enabled; m_momentVarianceFloor = i_varFloor; }
		bool getMomentSelection() const { return m_momentSelection; }
		float getMomentVarianceFloor() const { return m_momentVarianceFloor; }
		/// Auxiliary feature buffers (albedo, shading normal, depth, object id, ...) that gate the similar-patch selection (bcd_hip_denoise_guided_host): two
		/// patches stay similar only if their features agree as well, so nothing is averaged across a texture or geometry edge that the radiance statistics
		/// cannot see.  i_pFeatures: W x H x F, 1 <= F <= 8; i_pVariances: the variance of each pixel's feature MEAN, same size, or null; i_rFloors: one
		/// value per channel, finite and >= 0 (without variances: the squared tolerance of the channel; 0 switches the channel off); i_threshold: finite,
		/// >= 0, 1 = "one tolerance rms".  Non-owning pointers, like DenoiserInputs.  A null features pointer switches the gate off.  Added layers, the
		/// prefilter switches and the moment selection work as without it; one device only.  Beside neighbour frames: see setNeighbourGuideFeatures.
		void setGuideFeatures(const DeepImage<float>* i_pFeatures, const DeepImage<float>* i_pVariances, const std::vector<float>& i_rFloors, float i_threshold = 1.f)
		{
			m_pGuideFeatures = i_pFeatures;
			m_pGuideVariances = i_pFeatures ? i_pVariances : nullptr;
			m_guideFloors = i_rFloors;
			m_guideThreshold = i_threshold;
		}
		const DeepImage<float>* getGuideFeatures() const { return m_pGuideFeatures; }
		const DeepImage<float>* getGuideVariances() const { return m_pGuideVariances; }
		const std::vector<float>& getGuideFloors() const { return m_guideFloors; }
		float getGuideThreshold() const { return m_guideThreshold; }

		/// A neighbouring frame of the sequence (t - 1, t + 1, ...) that lends its statistics to the frame in DenoiserInputs (bcd_hip_denoise_temporal_host):
		/// similar patches are also searched in the same window of every neighbour frame, and mean, noise mean and covariance of the estimate come from the
		/// union of the sets; only the frame itself is denoised.  Each neighbour brings all four images, of the frame's width, height and histogram depth.
		/// Non-owning pointers, like DenoiserInputs.  At most 4 neighbours, patch radius 1 and search radius 6, one device; together with the spike
		/// prefilter only under setSpikePrefilterFrames(true); under the moment selection see addNeighbourFrameMoments; feature buffers need setNeighbourGuideFeatures for every neighbour.  With no neighbour denoise() is what it always was.
		void addNeighbourFrame(const DenoiserInputs& i_rFrame)
		{
			m_neighbourFrames.push_back(i_rFrame); m_neighbourLayers.emplace_back(); m_neighbourMotion.push_back(nullptr); m_neighbourGuides.emplace_back();
			m_neighbourMoments.push_back(0);
		}
		/// A neighbouring frame for the selection from means and covariances (setMomentSelection(true); bcd_hip_denoise_temporal_moments_host): colours, sample
		/// counts and sample covariances of the frame's size, m_pHistograms may be null and is not looked at.  addNeighbourFrameLayer, setNeighbourMotion and
		/// setNeighbourGuideFeatures index it like any other neighbour.  denoise() serves neighbour frames under the moment selection only when EVERY neighbour
		/// was added this way, refuses such neighbours without setMomentSelection(true), and keeps its refusal of addNeighbourFrame under the moment selection.
		void addNeighbourFrameMoments(const DenoiserInputs& i_rFrame)
		{
			addNeighbourFrame(i_rFrame);
			m_neighbourMoments.back() = 1;
		}
		void clearNeighbourFrames() { m_neighbourFrames.clear(); m_neighbourLayers.clear(); m_neighbourMotion.clear(); m_neighbourGuides.clear(); m_neighbourMoments.clear(); }
		/// per neighbour 1 when it was added by addNeighbourFrameMoments, else 0
		const std::vector<char>& getNeighbourMomentFlags() const { return m_neighbourMoments; }
		void setNeighbourMomentFlags(const std::vector<char>& i_rFlags) { m_neighbourMoments = i_rFlags; m_neighbourMoments.resize(m_neighbourFrames.size(), 0); }
		const std::vector<DenoiserInputs>& getNeighbourFrames() const { return m_neighbourFrames; }
		void setNeighbourFrames(const std::vector<DenoiserInputs>& i_rFrames)
		{
			m_neighbourFrames = i_rFrames;
			m_neighbourLayers.assign(i_rFrames.size(), std::vector<NeighbourLayer>());
			m_neighbourMotion.assign(i_rFrames.size(), nullptr);
			m_neighbourGuides.assign(i_rFrames.size(), NeighbourGuide());
			m_neighbourMoments.assign(i_rFrames.size(), 0);
		}
		/// The feature buffers of neighbour i_neighbour (bcd_hip_denoise_temporal_guided_host): with setGuideFeatures and neighbour frames, the gate that protects
		/// the search inside the frame protects the search in the neighbours too -- a patch of a neighbour stays similar only if its features agree with the
		/// frame's.  i_pFeatures: the frame's feature size and channel count; i_pVariances: given exactly when the frame's guide has variances.  Floors and
		/// threshold are those of setGuideFeatures.  A neighbour with a motion field has its features reprojected with its other images.  denoise() refuses a
		/// neighbour without features while setGuideFeatures is in force.  clearNeighbourFrames() clears all.  An index that names no neighbour is ignored.
		struct NeighbourGuide
		{
			const DeepImage<float>* m_pFeatures = nullptr;
			const DeepImage<float>* m_pVariances = nullptr;
		};
		void setNeighbourGuideFeatures(size_t i_neighbour, const DeepImage<float>* i_pFeatures, const DeepImage<float>* i_pVariances)
		{
			if(i_neighbour < m_neighbourGuides.size())
			{
				m_neighbourGuides[i_neighbour].m_pFeatures = i_pFeatures;
				m_neighbourGuides[i_neighbour].m_pVariances = i_pFeatures ? i_pVariances : nullptr;
			}
		}
		const std::vector<NeighbourGuide>& getNeighbourGuides() const { return m_neighbourGuides; }
		void setNeighbourGuides(const std::vector<NeighbourGuide>& i_rGuides) { m_neighbourGuides = i_rGuides; m_neighbourGuides.resize(m_neighbourFrames.size()); }
		/// The motion field of neighbour i_neighbour (bcd_hip_denoise_temporal_motion_host): a 2-channel image of the frame's size, (dx, dy) per pixel -- pixel
		/// (l, c) of the frame shows what pixel (l + round(dy), c + round(dx)) of the neighbour shows, rounding to nearest even; NaN marks a disoccluded pixel.
		/// The neighbour is reprojected into the frame's pixel grid before its similar patches are searched, and members whose patch holds a pixel without a
		/// source are left out.  nullptr clears the field (zero motion); clearNeighbourFrames() clears all.  An index that names no neighbour is ignored.
		void setNeighbourMotion(size_t i_neighbour, const DeepImage<float>* i_pMotion)
		{
			if(i_neighbour < m_neighbourMotion.size())
				m_neighbourMotion[i_neighbour] = i_pMotion;
		}
		const std::vector<const DeepImage<float>*>& getNeighbourMotions() const { return m_neighbourMotion; }
		void setNeighbourMotions(const std::vector<const DeepImage<float>*>& i_rMotions) { m_neighbourMotion = i_rMotions; m_neighbourMotion.resize(m_neighbourFrames.size(), nullptr); }
		/// Added layers beside neighbour frames (bcd_hip_denoise_temporal_layers_host): neighbour i_neighbour (the index in the order of addNeighbourFrame) brings
		/// the colours and sample covariances of one more layer; its k-th call pairs with the k-th addLayer.  denoise() accepts layers beside neighbours when
		/// every neighbour has exactly one such layer per addLayer, in the frame's size, and refuses anything else.  An index that names no neighbour is ignored.
		struct NeighbourLayer
		{
			const DeepImage<float>* m_pColors;
			const DeepImage<float>* m_pSampleCovariances;
		};
		void addNeighbourFrameLayer(size_t i_neighbour, const DeepImage<float>* i_pColors, const DeepImage<float>* i_pSampleCovariances)
		{
			if(i_neighbour < m_neighbourLayers.size())
			{
				NeighbourLayer layer = { i_pColors, i_pSampleCovariances };
				m_neighbourLayers[i_neighbour].push_back(layer);
			}
		}
		const std::vector<std::vector<NeighbourLayer>>& getNeighbourFrameLayers() const { return m_neighbourLayers; }
		void setNeighbourFrameLayers(const std::vector<std::vector<NeighbourLayer>>& i_rLayers) { m_neighbourLayers = i_rLayers; m_neighbourLayers.resize(m_neighbourFrames.size()); }

	protected:
		uint32_t m_orderSeed;
		std::vector<int> m_devices;
		float m_prefilterThresholdStDevFactor;
		bool m_zeroBadOutputValues;
		bool m_prefilterLayers;
		bool m_prefilterFrames;
		bool m_momentSelection;
		float m_momentVarianceFloor;
		const DeepImage<float>* m_pGuideFeatures;
		const DeepImage<float>* m_pGuideVariances;
		std::vector<float> m_guideFloors;
		float m_guideThreshold;
		std::vector<ColorLayer> m_layers;
		std::vector<DenoiserInputs> m_neighbourFrames;
		std::vector<std::vector<NeighbourLayer>> m_neighbourLayers; // [neighbour][added layer], as long as m_neighbourFrames
		std::vector<const DeepImage<float>*> m_neighbourMotion;     // [neighbour] its motion field or nullptr, as long as m_neighbourFrames
		std::vector<NeighbourGuide> m_neighbourGuides;              // [neighbour] its feature buffers, as long as m_neighbourFrames
		std::vector<char> m_neighbourMoments;                       // [neighbour] 1: added by addNeighbourFrameMoments, as long as m_neighbourFrames
	};

	/// The engine contexts behind denoise() (device workspaces, pyramids, staging buffers: grow-only, sized by the largest frame seen,
	/// one set per device / device list) live until the process ends so that a sequence of frames pays for them once.  A long-lived
	/// host application calls this to give the device memory back; the next denoise() builds what it needs again.  Thread safe; waits
	/// for calls in flight.
	void releaseEngines();

	class Denoiser : public IDenoiser, public HipEngineSettings
	{
	public:
		Denoiser() : IDenoiser(), m_width(0), m_height(0), m_nbOfPixels(0) {}
		virtual ~Denoiser() {}

	public:
		virtual bool denoise();

		/// null / empty / size-mismatch checks of the reference (src/core/Denoiser.cpp:238-348); prints to cerr
		bool inputsOutputsAreOk();
		/// the same for the added colour layers (sizes against the primary colour image)
		bool layersAreOk();
		/// ... and for the feature buffers of setGuideFeatures
		bool guideIsOk();

		int getImagesWidth() const { return m_width; }
		int getImagesHeight() const { return m_height; }

		/// the whole path for 1..n scales (MultiscaleDenoiser forwards here: the pyramid, the scales and the merges are one call
		/// into the engine)
		bool denoiseWithNbOfScales(int i_nbOfScales);

	private:
		int m_width;
		int m_height;
		int m_nbOfPixels;
	};

} // namespace bcd

#endif // DENOISER_H
