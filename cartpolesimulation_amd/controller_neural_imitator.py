"""controller_neural_imitator — the neural imitator of the MPC as a controller object, on the HIP path.

The reference's ``controller_neural_imitator`` lives in the Control_Toolkit submodule, which the reference checkout does not carry;
what is in the tree is the network it runs (GymlikeCartPole/Dense-7IN-32H1-32H2-1OUT-0/) and the controllers' common call shape
(``template_controller``: ``configure``, ``step(s, time, updated_attributes)`` -> the control).  This stand-in keeps that call shape
and nothing else of its own: ``configure(folder)`` reads the model folder (``model_folder.load_dense_model``) and hands it to the
engine, ``step`` is one ``MPPIEngine.dense_control`` with E = 1 on the state and the ``target_position`` / ``target_equilibrium``
attributes - clip to [-1, 1] included, which is the library's (include/cpmppi.h).  Many envs at once run in the device loop:
``harness.run_schedule(imitator=...)``, ``recording --imitator FOLDER``.
"""
import numpy as np

from .controller_mpc import template_controller


class controller_neural_imitator(template_controller):
    def __init__(self, environment_name="CartPole", initial_environment_attributes=None, control_limits=None, device=0, engine=None,
                 **kwargs):
        super().__init__(environment_name, initial_environment_attributes, control_limits)
        self.device, self.engine, self.model = device, engine, None

    def configure(self, folder_or_model):
        """``folder_or_model``: a Dense-7IN-32H1-32H2-1OUT-* model folder, or the dict ``MPPIEngine.set_dense`` takes."""
        from .engine import MPPIEngine
        from .harness import check_imitator
        self.model = check_imitator(folder_or_model)
        if self.engine is None:
            from .configs import MPPIConfig
            self.engine = MPPIEngine(1, MPPIConfig(num_rollouts=1, mpc_horizon=2), device=self.device)
        eng = self.engine
        eng.set_dense(self.model)
        self._s, self._tp, self._te = eng.zeros(1, 6), eng.zeros(1), eng.zeros(1)
        self._call = eng.prepare_dense_control(self._s, self._tp, self._te)
        return self

    def step(self, s, time=None, updated_attributes=None):
        self.update_attributes(updated_attributes)
        vp = self.variable_parameters
        self._s.copy_(self.engine.tensor(np.asarray(s, np.float32).reshape(1, 6)))
        self._tp.fill_(float(getattr(vp, "target_position", 0.0)))
        self._te.fill_(float(getattr(vp, "target_equilibrium", 1.0)))
        return float(self._call.run()[0][0])

    def controller_reset(self):
        pass                                                       # (the network has no memory)
