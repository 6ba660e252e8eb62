// policies.hpp -- MlpPolicy with the reference's method names (ppo2/policies.hpp:26-82).  The reference wraps
// tensorflow::Session::Run with fixed feed/fetch names; this one wraps the C-ABI of libppo_hip (include/ppo_hip.h).
// Results come back as Mats: step -> {actions [n,A], values [n,1], neglogps [n,1]}; a categorical handle (ppo_create_ex with
// PPO_ACT_CATEGORICAL, an Env whose action space is SPACE_DISCRETE) returns actions [n,1] holding the category index, a multi-categorical one (ppo_create_multi, an
// Env with the IMultiDiscrete mixin) actions [n,K] holding the index within every component.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ppo_hip.h"
#include "../mat.hpp"

class MlpPolicy {
public:
    explicit MlpPolicy(ppo_handle* handle, int act_dim) : h_(handle), act_dim_(action_width(handle, act_dim)) {}
    // columns of an action matrix: act_dim (Gaussian; multi-binary: the bits), 1 (categorical: the category index) or K (multi-categorical) -- what the handle reports (ppo_action_width)
    static int action_width(ppo_handle* handle, int act_dim) { return handle ? ppo_action_width(handle) : act_dim; }
    int action_width() const { return act_dim_; }
    virtual ~MlpPolicy() {}

    // output/_action, output/_value_flat, output/_neglogp  (policies.hpp:33-46); noise == nullptr: on-device RNG
    // mask [n, categories] (a categorical handle; env/action_mask.hpp): the action is sampled among the allowed categories; nullptr: unmasked
    virtual std::vector<Mat> step(const Mat& obs, const Mat* noise = nullptr, const Mat* mask = nullptr) {
        const int n = static_cast<int>(obs.rows());
        Mat a(n, act_dim_), v(n, 1), nlp(n, 1);
        check(ppo_step_masked(h_, obs.data(), n, noise ? noise->data() : nullptr, mask ? mask->data() : nullptr, a.data(), v.data(), nlp.data()), "step");
        return {a, v, nlp};
    }
    // output/_deterministic_action (policies.hpp:49-62); mask as in step(): the best ALLOWED category
    virtual Mat get_deterministic_action(const Mat& obs, const Mat* mask = nullptr) {
        Mat a(obs.rows(), act_dim_);
        check(ppo_act_deterministic_masked(h_, obs.data(), static_cast<int>(obs.rows()), mask ? mask->data() : nullptr, a.data()), "get_action()");
        return a;
    }
    // output/_value_flat (policies.hpp:64-77)
    virtual Mat value(const Mat& obs) {
        Mat v(obs.rows(), 1);
        check(ppo_value(h_, obs.data(), static_cast<int>(obs.rows()), v.data()), "value()");
        return v;
    }
    // The policy for GIVEN actions (no reference counterpart; stable-baselines 3 evaluate_actions): {values [n,1], neglogps [n,1], entropies [n,1]}.  actions as step()
    // returns them, mask as step() takes it.  Stateless: no draw, nothing of the rollout, the normaliser or Adam is touched (include/ppo_hip.h, ppo_evaluate_actions).
    virtual std::vector<Mat> evaluate_actions(const Mat& obs, const Mat& actions, const Mat* mask = nullptr) {
        const int n = static_cast<int>(obs.rows());
        if (actions.rows() != obs.rows() || actions.cols() != act_dim_) throw std::runtime_error("evaluate_actions error: actions must be [n, action_width]");
        Mat v(n, 1), nlp(n, 1), ent(n, 1);
        check(ppo_evaluate_actions(h_, obs.data(), actions.data(), n, mask ? mask->data() : nullptr, v.data(), nlp.data(), ent.data()), "evaluate_actions");
        return {v, nlp, ent};
    }
    // The action distribution's parameters [n, W] (stable-baselines 2 ActorCriticPolicy.proba_step): Gaussian mu | std, categorical / multi-categorical the
    // probabilities of every category (0 for a forbidden one), multi-binary P(bit = 1); W = ppo_distribution_width
    virtual Mat proba_step(const Mat& obs, const Mat* mask = nullptr) {
        const int n = static_cast<int>(obs.rows()), W = ppo_distribution_width(h_);
        Mat p(n, W);
        check(ppo_action_probability(h_, obs.data(), n, mask ? mask->data() : nullptr, p.data(), (int64_t)n * W), "proba_step");
        return p;
    }
    // Runner::set_returns' GAE scan (runner.hpp:159-191) on the device; [T,E] time-major
    virtual void gae(const Mat& rewards, const Mat& values, const Mat& dones, const Mat& last_values, const Mat& last_dones, float gamma,
                     float lam, Mat& returns) {
        check(ppo_gae(h_, rewards.data(), values.data(), dones.data(), last_values.data(), last_dones.data(), static_cast<int>(rewards.rows()),
                      static_cast<int>(rewards.cols()), gamma, lam, returns.data()), "gae");
    }
    // ... with the value bootstrap at time-limit truncations: terminal_values [T,E] = V(terminal observation) on the truncated rows, 0 elsewhere (ppo_gae_ex)
    virtual void gae_truncated(const Mat& rewards, const Mat& values, const Mat& dones, const Mat& last_values, const Mat& last_dones, const Mat& terminal_values,
                               float gamma, float lam, Mat& returns) {
        check(ppo_gae_ex(h_, rewards.data(), values.data(), dones.data(), last_values.data(), last_dones.data(), terminal_values.data(),
                         static_cast<int>(rewards.rows()), static_cast<int>(rewards.cols()), gamma, lam, returns.data()), "gae");
    }
    ppo_handle* handle() const { return h_; }

protected:
    MlpPolicy() : h_(nullptr), act_dim_(0) {}
    void check(int rc, const char* what) { if (rc != 0) throw std::runtime_error(std::string(what) + " error: " + ppo_last_error(h_)); }
    ppo_handle* h_;
    int act_dim_;
};
