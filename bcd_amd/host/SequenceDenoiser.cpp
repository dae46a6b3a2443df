// SequenceDenoiser.cpp -- bcd::SequenceDenoiser of the MI355X build: the checks that need no device, with messages on cerr in the style of
// Denoiser.cpp, then the host push and pop of the sequence object of the C ABI (bcd_hip_sequence_*, include/bcd_hip.h).  The object owns its engine
// context: the frames it keeps on the device live and die with it.
#include "SequenceDenoiser.h"

#include "DeepImage.h"
#include "bcd_hip.h"

#include <algorithm>
#include <iostream>
#include <limits>
#include <omp.h>
#include <vector>

using namespace std;

namespace bcd
{

	SequenceDenoiser::SequenceDenoiser(int i_nbOfScales, int i_temporalRadius) :
			m_nbOfScales(i_nbOfScales), m_temporalRadius(i_temporalRadius), m_pCtx(nullptr), m_pSequence(nullptr), m_width(0), m_height(0), m_depth(0),
			m_lastFrameIndex(-1), m_frameSettings(false), m_plain(true), m_nbOfLayers(1), m_moments(false), m_nbOfFeatures(0), m_featureVariances(false),
			m_pMotionPrev(nullptr), m_pMotionNext(nullptr)
	{
	}

	SequenceDenoiser::~SequenceDenoiser() { release(); }

	void SequenceDenoiser::release()
	{
		if(m_pSequence) bcd_hip_sequence_destroy(m_pSequence); // (before its context)
		if(m_pCtx) bcd_hip_ctx_destroy(static_cast<bcd_hip_ctx*>(m_pCtx));
		m_pSequence = nullptr;
		m_pCtx = nullptr;
	}

	void SequenceDenoiser::reset()
	{
		// (the sequence is created again by the next push: its size, scales, radius and parameters may have changed)
		if(m_pSequence) bcd_hip_sequence_destroy(m_pSequence);
		m_pSequence = nullptr;
		m_lastFrameIndex = -1;
	}

	bool SequenceDenoiser::settingsAreOk() const
	{
		if(m_temporalRadius < 1 || 2 * m_temporalRadius > BCD_HIP_MAX_NEIGHBOURS)
		{
			cerr << "Aborting denoising: the temporal radius of a sequence must be 1 or 2, not " << m_temporalRadius << endl;
			return false;
		}
		if(m_nbOfScales < 1)
		{
			cerr << "Aborting denoising: the number of scales must be at least 1" << endl;
			return false;
		}
		if(m_parameters.m_patchRadius != 1 || m_parameters.m_searchWindowRadius != 6)
		{
			cerr << "Aborting denoising: a sequence is denoised with patch radius 1 and search radius 6 (neighbour frames support no other geometry)" << endl;
			return false;
		}
		if(m_devices.size() > 1)
		{
			cerr << "Aborting denoising: a sequence is not available over several devices" << endl;
			return false;
		}
		if(!m_frameSettings && (!m_layers.empty() || !m_neighbourFrames.empty() || m_momentSelection || m_pGuideFeatures || (m_prefilterThresholdStDevFactor > 0.f && !m_prefilterFrames)))
		{
			cerr << "Aborting denoising: a sequence takes no added colour layers, no neighbour frames of its own (the window supplies them), no moment selection, no "
					"feature buffers and no spike prefilter" << endl;
			return false;
		}
		if(!m_neighbourFrames.empty() || (m_prefilterThresholdStDevFactor > 0.f && !m_prefilterFrames)) // (setSpikePrefilterFrames(true): every pushed frame is prefiltered once)
		{
			cerr << "Aborting denoising: a sequence takes no neighbour frames of its own (the window supplies them) and no spike prefilter" << endl;
			return false;
		}
		if(m_layers.size() + 1 > size_t(BCD_HIP_MAX_LAYERS))
		{
			cerr << "Aborting denoising: at most " << BCD_HIP_MAX_LAYERS - 1 << " added colour layers" << endl;
			return false;
		}
		if(m_momentSelection && (!(m_momentVarianceFloor >= 0.f) || !(m_momentVarianceFloor <= std::numeric_limits<float>::max())))
		{
			cerr << "Aborting denoising: the variance floor of the moment selection must be finite and not negative" << endl;
			return false;
		}
		if(m_pGuideFeatures)
		{
			const int f = m_pGuideFeatures->getDepth();
			if(m_pGuideFeatures->isEmpty() || f < 1 || f > BCD_HIP_GUIDE_MAX_CHANNELS)
			{
				cerr << "Aborting denoising: the feature image must have 1 to " << BCD_HIP_GUIDE_MAX_CHANNELS << " channels" << endl;
				return false;
			}
			if(int(m_guideFloors.size()) != f)
			{
				cerr << "Aborting denoising: one feature floor per feature channel expected (" << f << ", not " << m_guideFloors.size() << ")" << endl;
				return false;
			}
			bool counts = m_pGuideVariances != nullptr;
			for(float x : m_guideFloors)
			{
				if(!(x >= 0.f) || !(x <= std::numeric_limits<float>::max()))
				{
					cerr << "Aborting denoising: a feature floor must be finite and not negative" << endl;
					return false;
				}
				counts = counts || x > 0.f;
			}
			if(!(m_guideThreshold >= 0.f) || !(m_guideThreshold <= std::numeric_limits<float>::max()))
			{
				cerr << "Aborting denoising: the feature threshold must be finite and not negative" << endl;
				return false;
			}
			if(!counts)
			{
				cerr << "Aborting denoising: no feature channel can count: every floor is 0 and there are no variances" << endl;
				return false;
			}
		}
		return true;
	}

	bool SequenceDenoiser::frameIsOk(const DenoiserInputs& i_rFrame) const
	{
		const DeepImage<float>* images[4] = { i_rFrame.m_pColors, i_rFrame.m_pNbOfSamples, i_rFrame.m_pHistograms, i_rFrame.m_pSampleCovariances };
		const char* names[4] = { "color", "number of samples", "histogram", "covariance" };
		for(int i = 0; i < 4; ++i)
			if((i != 2 || !m_momentSelection) && (!images[i] || images[i]->isEmpty())) // (the moment selection looks at no histogram)
			{
				cerr << "Aborting denoising: nullptr or empty input " << names[i] << " image" << endl;
				return false;
			}
		const int w = images[0]->getWidth(), h = images[0]->getHeight();
		for(int i = 1; i < 4; ++i)
			if((i != 2 || !m_momentSelection) && (images[i]->getWidth() != w || images[i]->getHeight() != h))
			{
				cerr << "Aborting denoising: input " << names[i] << " image is " << images[i]->getWidth() << "x" << images[i]->getHeight()
						<< " but input color image is " << w << "x" << h << endl;
				return false;
			}
		if(images[0]->getDepth() != 3 || images[1]->getDepth() != 1 || images[3]->getDepth() != 6)
		{
			cerr << "Aborting denoising: expected depths 3 / 1 / 6 for color / number of samples / covariance images" << endl;
			return false;
		}
		for(size_t k = 0; k < m_layers.size(); ++k)
		{
			const DeepImage<float>* c = m_layers[k].m_pColors;
			const DeepImage<float>* v = m_layers[k].m_pSampleCovariances;
			if(!c || !v || c->getWidth() != w || c->getHeight() != h || c->getDepth() != 3 || v->getWidth() != w || v->getHeight() != h || v->getDepth() != 6)
			{
				cerr << "Aborting denoising: added layer " << k << " needs colours " << w << "x" << h << "x3 and covariances " << w << "x" << h << "x6" << endl;
				return false;
			}
		}
		if(m_pGuideFeatures)
		{
			if(m_pGuideFeatures->getWidth() != w || m_pGuideFeatures->getHeight() != h)
			{
				cerr << "Aborting denoising: the feature image is not " << w << "x" << h << endl;
				return false;
			}
			if(m_pGuideVariances && (m_pGuideVariances->getWidth() != w || m_pGuideVariances->getHeight() != h || m_pGuideVariances->getDepth() != m_pGuideFeatures->getDepth()))
			{
				cerr << "Aborting denoising: the feature variances do not have the size of the features" << endl;
				return false;
			}
		}
		const int depth = m_momentSelection ? 0 : images[2]->getDepth();
		if(m_pSequence && (w != m_width || h != m_height || depth != m_depth))
		{
			cerr << "Aborting denoising: every frame of a sequence has the size of its first frame (" << m_width << "x" << m_height << ", " << m_depth
					<< " histogram channels)" << endl;
			return false;
		}
		if(m_pSequence && (int(m_layers.size()) + 1 != m_nbOfLayers || m_momentSelection != m_moments || (m_pGuideFeatures ? m_pGuideFeatures->getDepth() : 0) != m_nbOfFeatures ||
				(m_pGuideVariances != nullptr) != m_featureVariances))
		{
			cerr << "Aborting denoising: every frame of a sequence has the layers, the selection and the feature buffers (with or without variances) of its first frame"
					<< endl;
			return false;
		}
		return true;
	}

	bool SequenceDenoiser::pushFrame(const DenoiserInputs& i_rFrame)
	{
		const Deepimf* motion[2] = { m_pMotionPrev, m_pMotionNext }; // (setFrameMotion serves this push only)
		m_pMotionPrev = m_pMotionNext = nullptr;
		if(!settingsAreOk() || !frameIsOk(i_rFrame))
			return false;
		for(int d = 0; d < 2; ++d)
			if(motion[d] && (motion[d]->getDepth() != 2 || motion[d]->getWidth() != i_rFrame.m_pColors->getWidth() || motion[d]->getHeight() != i_rFrame.m_pColors->getHeight()))
			{
				cerr << "Aborting denoising: the motion field of a frame towards the " << (d ? "next" : "previous") << " frame needs 2 channels and the frame's size ("
						<< i_rFrame.m_pColors->getWidth() << "x" << i_rFrame.m_pColors->getHeight() << "), not " << motion[d]->getWidth() << "x" << motion[d]->getHeight() << "x"
						<< motion[d]->getDepth() << endl;
				return false;
			}
		if(!m_pSequence)
		{
			const int w = i_rFrame.m_pColors->getWidth(), h = i_rFrame.m_pColors->getHeight(), depth = m_momentSelection ? 0 : i_rFrame.m_pHistograms->getDepth();
			for(int s = 1, ws = w, hs = h; s < m_nbOfScales; ++s)
			{
				ws /= 2; hs /= 2;
				if(ws < 3 || hs < 3)
				{
					cerr << "Aborting denoising: too many scales for this image size" << endl;
					return false;
				}
			}
			const bool prefilter = m_prefilterFrames && m_prefilterThresholdStDevFactor > 0.f;
			if(prefilter && (w < 3 || h < 3 || !(m_prefilterThresholdStDevFactor <= std::numeric_limits<float>::max())))
			{
				cerr << "Aborting denoising: the spike prefilter of every frame (setSpikePrefilterFrames) needs a finite factor and frames of at least 3x3 pixels" << endl;
				return false;
			}
			bcd_hip_params prm;
			bcd_hip_default_params(&prm);
			prm.hist_dist_threshold = m_parameters.m_histogramDistanceThreshold;
			prm.patch_radius = m_parameters.m_patchRadius;
			prm.search_radius = m_parameters.m_searchWindowRadius;
			prm.min_eigen_value = m_parameters.m_minEigenValue;
			// the visiting order of Denoiser::denoiseWithNbOfScales: a shuffle (-r 1), else -- more than one thread -- the strip list, else scanline
			const int nbOfCores = m_parameters.m_nbOfCores > 0 ? m_parameters.m_nbOfCores : std::max(1, omp_get_max_threads());
			prm.use_random_pixel_order = m_parameters.m_useRandomPixelOrder ? 1 : (nbOfCores > 1 && w <= 8191 && h <= 8191 ? 2 : 0);
			prm.marked_skip_probability = m_parameters.m_markedPixelsSkippingProbability;
			prm.order_seed = m_orderSeed;
			bcd_hip_ctx* pCtx = static_cast<bcd_hip_ctx*>(m_pCtx);
			if(!pCtx && bcd_hip_ctx_create(&pCtx, m_devices[0], nullptr) != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: no usable HIP device " << m_devices[0] << " (this build has no CPU path)" << endl;
				return false;
			}
			m_pCtx = pCtx;
			// the mode is that of the first frame: its layers (the frame's colours are layer 0), the selection, the feature buffers
			bcd_hip_sequence_mode mode = {};
			mode.nb_layers = int(m_layers.size()) + 1;
			mode.moments = m_momentSelection ? 1 : 0;
			mode.var_floor = m_momentVarianceFloor;
			mode.nb_features = m_pGuideFeatures ? m_pGuideFeatures->getDepth() : 0;
			mode.feature_variances = m_pGuideVariances ? 1 : 0;
			mode.feature_floors = m_pGuideFeatures ? m_guideFloors.data() : nullptr;
			mode.feature_threshold = m_guideThreshold;
			// (one layer, histograms, no gate: the sequence of bcd_hip_sequence_create with its push and pop -- made by bcd_hip_sequence_create_mode, which builds the
			// same object and also takes a later frame that brings motion fields)
			m_plain = mode.nb_layers == 1 && !mode.moments && mode.nb_features == 0;
			const int rc = bcd_hip_sequence_create_mode(pCtx, w, h, depth, m_nbOfScales, m_temporalRadius, &prm, &mode, &m_pSequence);
			if(rc != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: " << bcd_hip_last_error(pCtx) << endl;
				m_pSequence = nullptr;
				return false;
			}
			if(prefilter && bcd_hip_sequence_set_prefilter(m_pSequence, m_prefilterThresholdStDevFactor) != BCD_HIP_OK)
			{	// (the factor of the first frame serves the sequence, like its mode)
				cerr << "Aborting denoising: " << bcd_hip_last_error(pCtx) << endl;
				bcd_hip_sequence_destroy(m_pSequence);
				m_pSequence = nullptr;
				return false;
			}
			m_nbOfLayers = mode.nb_layers; m_moments = m_momentSelection; m_nbOfFeatures = mode.nb_features; m_featureVariances = mode.feature_variances != 0;
			m_width = w; m_height = h; m_depth = depth;
			m_lastFrameIndex = -1;
		}
		int rc;
		if(m_plain && !motion[0] && !motion[1])
			rc = bcd_hip_sequence_push_host(m_pSequence, i_rFrame.m_pColors->getDataPtr(), i_rFrame.m_pNbOfSamples->getDataPtr(), i_rFrame.m_pHistograms->getDataPtr(),
					i_rFrame.m_pSampleCovariances->getDataPtr());
		else
		{
			std::vector<bcd_hip_frame_layer> layers(m_nbOfLayers);
			layers[0] = { i_rFrame.m_pColors->getDataPtr(), i_rFrame.m_pSampleCovariances->getDataPtr() };
			for(size_t k = 0; k < m_layers.size(); ++k)
				layers[k + 1] = { m_layers[k].m_pColors->getDataPtr(), m_layers[k].m_pSampleCovariances->getDataPtr() };
			bcd_hip_sequence_frame frame = {};
			frame.nsamples = i_rFrame.m_pNbOfSamples->getDataPtr();
			frame.histograms = m_moments ? nullptr : i_rFrame.m_pHistograms->getDataPtr();
			frame.layers = layers.data();
			frame.features = m_pGuideFeatures ? m_pGuideFeatures->getDataPtr() : nullptr;
			frame.variances = m_pGuideVariances ? m_pGuideVariances->getDataPtr() : nullptr;
			rc = motion[0] || motion[1] ? bcd_hip_sequence_push_frame_motion_host(m_pSequence, &frame, motion[0] ? motion[0]->getDataPtr() : nullptr,
							motion[1] ? motion[1]->getDataPtr() : nullptr)
					: bcd_hip_sequence_push_frame_host(m_pSequence, &frame);
		}
		if(rc != BCD_HIP_OK)
		{
			cerr << "Aborting denoising: " << bcd_hip_last_error(static_cast<bcd_hip_ctx*>(m_pCtx)) << endl;
			return false;
		}
		return true;
	}

	bool SequenceDenoiser::end()
	{
		if(!m_pSequence)
		{
			cerr << "Aborting denoising: no frame has been pushed" << endl;
			return false;
		}
		return bcd_hip_sequence_end(m_pSequence) == BCD_HIP_OK;
	}

	int SequenceDenoiser::ready() const { return m_pSequence ? bcd_hip_sequence_ready(m_pSequence) : 0; }

	bool SequenceDenoiser::popFrame(DenoiserOutputs& o_rOutputs)
	{
		if(!o_rOutputs.m_pDenoisedColors)
		{
			cerr << "Aborting denoising: nullptr for output image" << endl;
			return false;
		}
		if(ready() < 1)
		{
			cerr << "Aborting denoising: no frame of the sequence is ready (push its later neighbours, or call end())" << endl;
			return false;
		}
		if(int(m_layers.size()) + 1 != m_nbOfLayers)
		{
			cerr << "Aborting denoising: the sequence has " << m_nbOfLayers - 1 << " added layers: as many must be registered when a frame is popped (their outputs are written)" << endl;
			return false;
		}
		for(const ColorLayer& l : m_layers)
			if(!l.m_pDenoisedColors)
			{
				cerr << "Aborting denoising: nullptr for the output image of an added layer" << endl;
				return false;
			}
		Deepimf result(m_width, m_height, 3);
		std::vector<Deepimf> more(m_layers.size(), Deepimf(m_width, m_height, 3));
		int64_t index = -1;
		int rc;
		if(m_plain)
			rc = bcd_hip_sequence_pop_host(m_pSequence, result.getDataPtr(), &index);
		else
		{
			std::vector<float*> outs(1, result.getDataPtr());
			for(Deepimf& m : more) outs.push_back(m.getDataPtr());
			rc = bcd_hip_sequence_pop_layers_host(m_pSequence, outs.data(), m_nbOfLayers, &index);
		}
		if(rc != BCD_HIP_OK)
		{
			cerr << "Aborting denoising: " << bcd_hip_last_error(static_cast<bcd_hip_ctx*>(m_pCtx)) << endl;
			return false;
		}
		if(m_zeroBadOutputValues)
			for(int k = 0; k < m_nbOfLayers; ++k)
			{
				float* p = k ? more[k - 1].getDataPtr() : result.getDataPtr();
				for(size_t i = 0, n = size_t(m_width) * m_height * 3; i < n; ++i)
					if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
						p[i] = 0.f;
			}
		for(size_t k = 0; k < m_layers.size(); ++k) *m_layers[k].m_pDenoisedColors = std::move(more[k]);
		*o_rOutputs.m_pDenoisedColors = std::move(result);
		m_lastFrameIndex = index;
		return true;
	}

} // namespace bcd
