// SequenceDenoiser.h -- the frames of an animation denoised through a sliding window (MI355X build; bcd_hip_sequence_* of include/bcd_hip.h).
// Denoiser::addNeighbourFrame denoises one frame with its neighbours and forgets everything: called once per frame of an animation it uploads every frame,
// builds its pyramid and searches every pair of frames 2 R + 1 times.  A SequenceDenoiser takes the frames one by one, keeps the last 2 R + 1 on the
// device, and hands back frame t denoised with the frames t - R .. t + R that exist -- what a Denoiser / MultiscaleDenoiser with those neighbours added in
// ascending order returns for it -- with every frame uploaded once and every pair of frames searched once.
#ifndef SEQUENCE_DENOISER_H
#define SEQUENCE_DENOISER_H

#include "Denoiser.h"

#include <cstdint>
#include <string>

namespace bcd
{

	/// Usage: setParameters / setOrderSeed / setDevice as on a Denoiser, then per frame pushFrame(), and popFrame() while ready() > 0; after the last frame
	/// end(), and popFrame() until ready() is 0.  Frame t can be popped once frame t + R is pushed, or after end(); a push is refused while the window is
	/// full (pop first).
	/// After setFrameSettings(true), colour layers, the moment selection and feature buffers have the semantics of HipEngineSettings, per pushed frame:
	///  - addLayer / setLayers: the layers registered when pushFrame() is called are that frame's added layers (colours and covariances are read; the
	///    DenoiserInputs colours are layer 0); the layers registered when popFrame() is called receive the popped frame's outputs in m_pDenoisedColors;
	///  - setMomentSelection(true, floor): every selection from means and covariances; DenoiserInputs::m_pHistograms may stay null and is not looked at;
	///  - setGuideFeatures: the features (and variances) set when pushFrame() is called are that frame's; floors and threshold are those of the first frame.
	/// The first frame fixes the mode: the number of layers, the selection, the feature channels and whether there are variances; reset() frees it.
	/// setFrameMotion(prev, next) gives the next pushed frame its motion fields towards the frame before and after it (bcd_hip_sequence_push_frame_motion): a
	/// neighbour whose direction has a field is warped into the frame's pixel grid, fields two frames away are composed from the steps.
	/// The settings a sequence does not serve -- neighbour frames of its own, setNeighbourMotion, the spike prefilter without setSpikePrefilterFrames(true) (with it every
	/// pushed frame is prefiltered once, on its own: bcd_hip_sequence_set_prefilter), several devices -- make pushFrame() return
	/// false, like a patch radius other than 1, a search radius other than 6, a temporal radius outside 1 .. 2, more than 15 added layers, a feature image
	/// outside 1 .. 8 channels, floors that are negative, not finite, of another count or unable to count, a frame that differs from the first frame's
	/// mode; every refusal comes before any device is asked for, with a message on cerr.
	class SequenceDenoiser : public HipEngineSettings
	{
	public:
		SequenceDenoiser(int i_nbOfScales = 1, int i_temporalRadius = 1);
		~SequenceDenoiser();
		SequenceDenoiser(const SequenceDenoiser&) = delete;
		SequenceDenoiser& operator=(const SequenceDenoiser&) = delete;

		const DenoiserParameters& getParameters() const { return m_parameters; }
		/// copied when the first frame is pushed; later changes take effect after reset()
		void setParameters(const DenoiserParameters& i_rParameters) { m_parameters = i_rParameters; }
		int getNbOfScales() const { return m_nbOfScales; }
		int getTemporalRadius() const { return m_temporalRadius; }
		/// true: added layers, the moment selection and feature buffers are taken per pushed frame, as described above.  false (default): a sequence with any
		/// of them set is refused with the message it always had -- one colour layer, histogram selection, no gate
		void setFrameSettings(bool i_enabled) { m_frameSettings = i_enabled; }
		bool getFrameSettings() const { return m_frameSettings; }

		/// the motion fields of the NEXT pushFrame(), which clears them: i_pPrev the field of that frame towards the frame before it, i_pNext towards the frame
		/// after it, (dx, dy) per pixel as in HipEngineSettings::setNeighbourMotion; nullptr: zero motion.  A field needs 2 channels and the frame's size:
		/// anything else makes pushFrame() return false with a message, before a device is asked for.  The images are read by pushFrame()
		void setFrameMotion(const Deepimf* i_pPrev, const Deepimf* i_pNext) { m_pMotionPrev = i_pPrev; m_pMotionNext = i_pNext; }
		/// the next frame: the four images are uploaded before the call returns.  The first frame fixes width, height and histogram depth
		bool pushFrame(const DenoiserInputs& i_rFrame);
		/// no further frame follows: the frames still held become ready
		bool end();
		/// frames that popFrame() can deliver now
		int ready() const;
		/// the next frame in push order; o_rOutputs.m_pDenoisedColors is resized to W x H x 3 and overwritten
		bool popFrame(DenoiserOutputs& o_rOutputs);
		/// index (from 0, in push order) of the frame the last successful popFrame() delivered, -1 before
		int64_t getLastFrameIndex() const { return m_lastFrameIndex; }
		/// forgets every frame (the device buffers stay) and takes the current parameters and settings for the next sequence
		void reset();

		/// the checks of pushFrame() that need no device, without the push (what bcd_cli runs on its arguments)
		bool settingsAreOk() const;

	private:
		bool frameIsOk(const DenoiserInputs& i_rFrame) const;
		void release();

		DenoiserParameters m_parameters;
		int m_nbOfScales;
		int m_temporalRadius;
		void* m_pCtx;      // bcd_hip_ctx of this object (created by the first push)
		void* m_pSequence; // bcd_hip_sequence_* handle
		int m_width, m_height, m_depth;
		int64_t m_lastFrameIndex;
		bool m_frameSettings;  // setFrameSettings
		// the mode of the sequence in progress (that of its first frame)
		bool m_plain;          // one layer, histograms, no feature gate: bcd_hip_sequence_create and its push and pop
		int m_nbOfLayers;
		bool m_moments;
		int m_nbOfFeatures;
		bool m_featureVariances;
		const Deepimf* m_pMotionPrev; // setFrameMotion: of the next push
		const Deepimf* m_pMotionNext;
	};

} // namespace bcd

#endif // SEQUENCE_DENOISER_H
